"""The optimizer's entry points bind through _lib from include/msm_hip.h alone, and the built library carries the bumped ABI
version.  Needs the built library, not a GPU: nothing is launched."""
from ctypes import c_float, c_int, c_void_p

from unseenobjectswithmeanshift_amd import _lib

P, I = c_void_p, c_int


def test_entry_points_bind_by_the_type_rule():
    sig, params = _lib._SIGNATURES, _lib._HEADER.params
    assert sig["msm_optim_grad_norm"] == (I, [P, P, P, P, I, I, P])
    assert sig["msm_optim_adamw_step"] == (I, [P, P, P, P, P, I, I, I, c_float, P])
    assert sig["msm_optim_zero"] == (I, [P, P, I, I, P])
    assert sig["msm_optim_chunk"] == (I, [])
    assert params["msm_optim_adamw_step"] == ["tensors", "chunks", "hyper", "partials", "state", "n_tensors", "n_chunks", "n_rows",
                                              "max_norm", "stream"]
    assert {"msm_optim_grad_norm", "msm_optim_adamw_step", "msm_optim_zero"} <= set(_lib.CallTimer.timed_entry_points())
    assert "msm_optim_chunk" not in _lib.CallTimer.timed_entry_points()


def test_library_carries_the_bumped_abi_and_the_chunk_of_the_header():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    L = _lib.lib()
    assert L.msm_abi_version() == _lib.ABI_VERSION == _lib.parse_header(text).abi_version and _lib.ABI_VERSION >= 37
    assert all(hasattr(L, n) for n in ("msm_optim_grad_norm", "msm_optim_adamw_step", "msm_optim_zero", "msm_optim_chunk"))
    from unseenobjectswithmeanshift_amd import ops
    assert ops.optim_chunk() == L.msm_optim_chunk() == _lib._define(text, "MSM_OPTIM_CHUNK") == 8192
    assert ops.OPTIM_ALIGNED == _lib._define(text, "MSM_OPTIM_ALIGNED") and ops.OPTIM_ALIGNED_G == _lib._define(text, "MSM_OPTIM_ALIGNED_G")


def test_bad_tables_are_refused_before_any_launch():
    L = _lib.lib()
    assert L.msm_optim_zero(None, None, 1, 1, None) != 0 and b"null pointer" in L.msm_last_error_string()
    assert L.msm_optim_zero(c_void_p(8), c_void_p(16), 2, 1, None) != 0 and b"every tensor has a chunk" in L.msm_last_error_string()
    assert L.msm_optim_grad_norm(c_void_p(8), c_void_p(12), c_void_p(8), c_void_p(8), 1, 1, None) != 0
    assert b"8-byte aligned" in L.msm_last_error_string()
    assert L.msm_optim_adamw_step(c_void_p(8), c_void_p(8), c_void_p(8), None, c_void_p(8), 1, 1, 1, c_float(0.01), None) != 0
    assert b"partials" in L.msm_last_error_string()
