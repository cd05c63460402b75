"""The ctypes bindings are read from include/msm_hip.h (_lib.parse_header): literal expectations for real prototypes that
between them use every type rule, the option names, the parser's strictness and robustness on synthetic headers, and the
entry points CallTimer brackets.  Pure Python: neither the library nor a GPU is needed."""
from ctypes import c_char_p, c_float, c_int, c_int64, c_uint64, c_void_p

import pytest

from unseenobjectswithmeanshift_amd import _lib

P, I, L, F = c_void_p, c_int, c_int64, c_float


@pytest.mark.parametrize("name, restype, argtypes", [
    ("msm_gemm_f32", I, [P] * 5 + [I] * 4 + [L] * 9 + [I] * 7 + [P]),                                  # nine int64_t, void* stream
    ("msm_ms_select_seeds", I, [P, I, I, I, I, P, L, P, P, P, L, I, c_uint64, P]),                     # the only uint64_t
    ("msm_layernorm_f32", I, [P, P, I, L, P, P, P, I, P, P, P, P, I, I, F, P]),                        # float eps
    ("msm_last_error_string", c_char_p, []),
    ("msm_abi_version", I, []),                                                                        # (void)
    ("msm_hypersphere_attn_workspace", L, [I, I, I, I]),                                               # int64_t return
    ("msm_groupnorm_nchw_pool_f32", I, [P] * 5 + [I] * 5 + [F, I, I] + [P, P, P, P, L, P]),            # float* const*, host const int32_t*
    ("msm_dec_set_prefetch", I, [P, P, I]),                                                            # const void* const*
], ids=lambda v: v if isinstance(v, str) else "")
def test_real_prototypes_bind_by_the_type_rule(name, restype, argtypes):
    res, args = _lib._SIGNATURES[name]
    assert res is restype
    assert len(args) == len(argtypes) and all(a is b for a, b in zip(args, argtypes)), args


def test_parameter_names_come_with_the_signatures():
    params = _lib._HEADER.params
    assert list(params) == list(_lib._SIGNATURES) and all(len(params[n]) == len(_lib._SIGNATURES[n][1]) for n in params)
    assert params["msm_abi_version"] == [] and params["msm_dec_set_prefetch"] == ["ptrs", "bytes", "n"]
    assert params["msm_layernorm_f32"][-2:] == ["eps", "stream"]
    assert params["msm_groupnorm_nchw_pool_f32"][13:] == ["th", "tw", "out", "zero_buf", "zero_count", "stream"]


def test_module_attributes_are_the_header():
    with open(_lib.HEADER_PATH) as f:
        h = _lib.parse_header(f.read())
    assert h.signatures == _lib._SIGNATURES and h.options == _lib.OPTIONS
    assert (h.abi_version, h.opt_auto) == (_lib.ABI_VERSION, _lib.OPT_AUTO)
    assert isinstance(_lib._SIGNATURES, dict) and isinstance(_lib.OPTIONS, tuple) and all(type(o) is str for o in _lib.OPTIONS)
    assert _lib.OPTIONS[0] == "MASK_NC" and _lib.OPTIONS[-1] == "GN_POOL" and "COUNT" not in _lib.OPTIONS
    assert _lib.OPT_AUTO == -1 and type(_lib.ABI_VERSION) is int


def header(body, enum="MSM_OPT_A = 0,\n    MSM_OPT_B,\n    MSM_OPT_COUNT"):
    """A minimal well-formed header around `body`."""
    return ('/* synthetic */\n#ifndef H\n#define H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
            "#define MSM_ABI_VERSION 7\n#define MSM_OPT_AUTO (-1)\nenum {\n    %s\n};\n%s\n"
            "#ifdef __cplusplus\n}\n#endif\n#endif /* H */\n" % (enum, body))


def test_synthetic_header_parses():
    h = _lib.parse_header(header("int msm_a(const float* x, int n, void* stream);\nint64_t msm_b(void);"))
    assert h.signatures == {"msm_a": (I, [P, I, P]), "msm_b": (L, [])}
    assert h.params == {"msm_a": ["x", "n", "stream"], "msm_b": []}
    assert (h.options, h.abi_version, h.opt_auto) == (("A", "B"), 7, -1)


@pytest.mark.parametrize("body, offender", [
    ("int msm_f(const float* x, size_t n, void* stream);", r"msm_f.*size_t"),
    ("int msm_g(double x);", r"msm_g.*double"),
    ("void msm_h(int n);", r"msm_h.*void"),
    ("float* msm_p(int n);", r"msm_p.*float \*"),
    ("int msm_u(int, int b);", r"msm_u.*`int`"),
    ("int msm_ok(int n);\ntypedef struct msm_ctx msm_ctx_t;", r"typedef struct msm_ctx msm_ctx_t"),
    ("int msm_ok(int n);\nint msm_cb(void (*fn)(int), int n);", r"msm_cb"),
    ("int msm_ok(int n);\nint msm_ok(int n);", r"msm_ok.*twice"),
    ("int msm_ok(int n);\nint msm_open(int n)", r"msm_open"),
], ids=["size_t", "double", "void_return", "pointer_return", "unnamed", "not_a_prototype", "function_pointer", "twice", "no_semicolon"])
def test_what_the_rule_does_not_cover_raises_and_is_named(body, offender):
    with pytest.raises(ValueError, match=offender):
        _lib.parse_header(header(body))


@pytest.mark.parametrize("enum, offender", [
    ("MSM_OPT_A = 0,\n    MSM_OPT_B = 5,\n    MSM_OPT_COUNT", r"MSM_OPT_B = 5"),
    ("MSM_OPT_A = 1,\n    MSM_OPT_B,\n    MSM_OPT_COUNT", r"MSM_OPT_A = 1"),
    ("MSM_OPT_A,\n    MSM_OPT_B", r"MSM_OPT_COUNT"),
    ("MSM_OPT_A,\n    OTHER_B,\n    MSM_OPT_COUNT", r"OTHER_B"),
], ids=["value", "first_not_zero", "no_count", "foreign_name"])
def test_option_keys_must_be_positions(enum, offender):
    with pytest.raises(ValueError, match=offender):
        _lib.parse_header(header("int msm_ok(int n);", enum))


def test_a_missing_define_raises():
    with pytest.raises(ValueError, match="MSM_ABI_VERSION"):
        _lib.parse_header(header("int msm_ok(int n);").replace("#define MSM_ABI_VERSION 7\n", ""))


def test_layout_and_comments_do_not_matter():
    body = ("int\nmsm_split(const float* const* w,\n          int64_t\n          stride,   // not msm_fake3(int);\n          void* stream\n);\n"
            "/* msm_fake(int); */\n"
            "#define MSM_FLAG 4   /* a changelog; with (parentheses); and int msm_fake2(int n); inside,\n   over two lines; */\n"
            "#define MSM_MACRO(x) \\\n    msm_fake4(x);\n"
            "const  char *msm_text( void );")
    h = _lib.parse_header(header(body))
    assert h.signatures == {"msm_split": (I, [P, L, P]), "msm_text": (c_char_p, [])}
    assert h.params["msm_split"] == ["w", "stride", "stream"]


def test_call_timer_brackets_exactly_the_stream_entry_points():
    sig, params = _lib._SIGNATURES, _lib._HEADER.params
    timed = _lib.CallTimer.timed_entry_points()
    assert timed == [n for n in sig if params[n] and params[n][-1] == "stream"] and len(timed) >= 100
    assert not any("stream" in params[n][:-1] for n in sig)
    assert not any(n.endswith("_workspace") for n in timed)
    assert all(sig[n][1][-1] is c_void_p for n in timed)
    # the rule this one replaced: last argument a pointer, name not *_workspace
    assert timed == [n for n in sig if sig[n][1] and sig[n][1][-1] is c_void_p and not n.endswith("_workspace")]
    assert "msm_dec_set_prefetch" not in timed and "msm_gemm_f32" in timed
