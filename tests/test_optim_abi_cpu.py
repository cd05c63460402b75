"""The optimizer's entry points bind through _lib from include/msm_hip.h alone, and the built library carries the bumped ABI
version and no longer the host-counted AdamW pair.  Needs the built library, not a GPU: nothing is launched.  (The signatures and
the other refusals of msm_optim_count_norm / msm_optim_update are held by tests/test_optim_rules_cpu.py.)"""
from ctypes import c_int, c_void_p

from unseenobjectswithmeanshift_amd import _lib

P, I = c_void_p, c_int
REMOVED = ("msm_optim_grad_norm", "msm_optim_adamw_step")          # ABI 37 .. 43


def test_entry_points_bind_by_the_type_rule():
    sig = _lib._SIGNATURES
    assert sig["msm_optim_zero"] == (I, [P, P, I, I, P])
    assert sig["msm_optim_chunk"] == (I, [])
    timed = set(_lib.CallTimer.timed_entry_points())
    assert {"msm_optim_count_norm", "msm_optim_update", "msm_optim_zero"} <= timed and "msm_optim_chunk" not in timed


def test_library_carries_the_bumped_abi_and_the_chunk_of_the_header():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    L = _lib.lib()
    assert L.msm_abi_version() == _lib.ABI_VERSION == _lib.parse_header(text).abi_version and _lib.ABI_VERSION > 43
    assert all(hasattr(L, n) for n in ("msm_optim_count_norm", "msm_optim_update", "msm_optim_zero", "msm_optim_chunk"))
    assert not any(n in _lib.declared_symbols() or n in _lib._SIGNATURES or hasattr(L, n) for n in REMOVED)
    from unseenobjectswithmeanshift_amd import ops
    assert ops.optim_chunk() == L.msm_optim_chunk() == _lib._define(text, "MSM_OPTIM_CHUNK") == 8192
    assert ops.OPTIM_ALIGNED == _lib._define(text, "MSM_OPTIM_ALIGNED") and ops.OPTIM_ALIGNED_G == _lib._define(text, "MSM_OPTIM_ALIGNED_G")


def test_bad_tables_are_refused_before_any_launch():
    L = _lib.lib()
    assert L.msm_optim_zero(None, None, 1, 1, None) != 0 and b"null pointer" in L.msm_last_error_string()
    assert L.msm_optim_zero(c_void_p(8), c_void_p(16), 2, 1, None) != 0 and b"every tensor has a chunk" in L.msm_last_error_string()
    assert L.msm_optim_count_norm(P(8), P(12), P(8), P(8), None, None, 1, 1, 1, None) != 0
    assert b"8-byte aligned" in L.msm_last_error_string()
