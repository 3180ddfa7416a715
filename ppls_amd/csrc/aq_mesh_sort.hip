// aq_mesh_sort.hip -- rocPRIM's radix sort of (double key, index) pairs for the accepted mesh (aq_mesh_sort.h), and
// of (row, index) pairs for the batch of meshes.
// <cstring> and <cstdlib> come first: included after rocPRIM's headers, memset and friends resolve to the
// device overloads inside them.
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "aq_mesh_sort.h"

namespace aq {

size_t mesh_sort_scratch_bytes(size_t n, hipError_t* err) {
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, (const double*)nullptr, (double*)nullptr,
                                                   (const unsigned*)nullptr, (unsigned*)nullptr, n);
    if (err) *err = e;
    return e == hipSuccess ? bytes : 0;
}

hipError_t mesh_sort(void* scratch, size_t scratch_bytes, const double* keys_in, double* keys_out,
                     const unsigned* idx_in, unsigned* idx_out, size_t n, hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, scratch_bytes, keys_in, keys_out, idx_in, idx_out, n, 0u, 64u, stream);
}

size_t mesh_sort_rows_scratch_bytes(size_t n, unsigned bits, hipError_t* err) {
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
                                                   (const unsigned*)nullptr, (unsigned*)nullptr, n, 0u, bits);
    if (err) *err = e;
    return e == hipSuccess ? bytes : 0;
}

hipError_t mesh_sort_rows(void* scratch, size_t scratch_bytes, const unsigned* rows_in, unsigned* rows_out,
                          const unsigned* idx_in, unsigned* idx_out, size_t n, unsigned bits, hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, scratch_bytes, rows_in, rows_out, idx_in, idx_out, n, 0u, bits, stream);
}

}  // namespace aq
