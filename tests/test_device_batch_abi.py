"""The device-resident batch's two entry points without a GPU: declared, exported, bound, and refusing on the
host -- before any device call -- what no context can be given for. (With a context, the other host-checked
arguments: tests/test_gpu_device_batch.py.)"""
import ctypes
import re
import subprocess

import pytest

NAMES = ["aq_integrate_batch_device", "aq_device_batch_check"]
AQ_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from ppls_amd import _lib
    return _lib.load()


def test_declared_bound_and_exported(lib):
    from test_abi import header_functions
    from ppls_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert name in header_functions() and name in _lib.EXPORTS and name in exported
        assert getattr(lib, name).restype is ctypes.c_int


def test_struct_layout_is_the_headers():
    """aq_device_io: nine device pointers, max_depth, reserved -- 80 bytes, as the C declaration lays it out."""
    from ppls_amd import _lib
    assert [f[0] for f in _lib.aq_device_io._fields_] == ["a", "b", "theta", "area", "accepted", "tasks", "err_abs",
                                                          "err_signed", "status", "max_depth", "reserved"]
    assert ctypes.sizeof(_lib.aq_device_io) == 80 and _lib.aq_device_io.max_depth.offset == 72
    src = open(_lib.HERE + "/../include/aquad.h").read()
    for name, bit in (("TIMEOUT", 1), ("OVERFLOW", 2), ("DEPTH", 4), ("INVALID", 8)):
        assert re.search(r"#define AQ_ROW_%s\s+%du\b" % (name, bit), src)
    from ppls_amd import aquad
    assert (aquad.ROW_TIMEOUT, aquad.ROW_OVERFLOW, aquad.ROW_DEPTH, aquad.ROW_INVALID) == (1, 2, 4, 8)


def test_null_context_is_refused_on_the_host(lib):
    from ppls_amd import _lib
    io = _lib.aq_device_io(max_depth=0)
    stream = ctypes.c_void_p(None)
    for n in (0, 1, 1 << 20):
        for s in (None, ctypes.byref(stream)):
            assert lib.aq_integrate_batch_device(None, n, ctypes.byref(io), 1e-6, 0, s) == AQ_EINVAL
            assert lib.aq_integrate_batch_device(None, n, None, 1e-6, 0, s) == AQ_EINVAL
    assert lib.aq_integrate_batch_device(None, 1, ctypes.byref(io), -1.0, 0, None) == AQ_EINVAL
    assert lib.aq_integrate_batch_device(None, 1, ctypes.byref(io), 1e-6, 7, None) == AQ_EINVAL
    count = ctypes.c_uint64(5)
    assert lib.aq_device_batch_check(None, ctypes.byref(count)) == AQ_EINVAL
    assert lib.aq_device_batch_check(None, None) == AQ_EINVAL


def test_import_stays_torch_free():
    """`import ppls_amd` (and loading the library) must not import torch: integrate_batch_device imports it itself."""
    import sys
    code = "import sys, ppls_amd; from ppls_amd import _lib; _lib.load(); assert 'torch' not in sys.modules; " \
           "assert ppls_amd.DeviceBatch._fields == ('area', 'tasks', 'accepted', 'err_abs', 'err_signed', 'status')"
    from ppls_amd import _lib
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=_lib.HERE + "/..", timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
