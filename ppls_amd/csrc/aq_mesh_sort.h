// aq_mesh_sort.h -- the accepted mesh's one sort: leaf keys (the leaves' left bounds: doubles of either sign,
// unique) with their indices, ascending. A translation unit of its own (aq_mesh_sort.hip) because it is the only
// user of rocPRIM, whose headers the kernels' file does not need to read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace aq {

// Bytes of scratch mesh_sort needs for n pairs (0 on failure, with *err set).
size_t mesh_sort_scratch_bytes(size_t n, hipError_t* err);
// keys_in / idx_in -> keys_out / idx_out (n pairs, no overlap), enqueued on `stream`. A radix sort: for unique
// keys the result does not depend on the schedule.
hipError_t mesh_sort(void* scratch, size_t scratch_bytes, const double* keys_in, double* keys_out,
                     const unsigned* idx_in, unsigned* idx_out, size_t n, hipStream_t stream);

// The batch of meshes' second pass (aq_integrate_mesh_batch): the rows of the l-sorted leaves as keys, over bits
// [0, bits), with the leaf indices as values. The sort is stable, so equal rows keep their l order: (row, l).
size_t mesh_sort_rows_scratch_bytes(size_t n, unsigned bits, hipError_t* err);
hipError_t mesh_sort_rows(void* scratch, size_t scratch_bytes, const unsigned* rows_in, unsigned* rows_out,
                          const unsigned* idx_in, unsigned* idx_out, size_t n, unsigned bits, hipStream_t stream);

}  // namespace aq
