"""ctypes binding of libmsm_hip.so, read from its C header.

include/msm_hip.h is the only description of the C ABI: ``parse_header`` turns its prototypes into the ctypes signatures, its
MSM_OPT_* enum into ``OPTIONS`` and its ``#define MSM_ABI_VERSION`` into ``ABI_VERSION``, once, when this module is imported.
A new entry point is declared in the header, defined in csrc/ and announced by a bump of MSM_ABI_VERSION; there is no second
place to edit.  Type rule: a parameter with a ``*`` is a ``c_void_p`` (device and host pointers alike), ``int`` / ``int64_t`` /
``uint64_t`` / ``float`` by value are the ctypes type of that name, ``const char*`` is the one pointer return type
(``c_char_p``); anything else in the header is an error, not a guess.

The product path has no CPU fallback: if the shared library is missing or a call fails, a
RuntimeError is raised (the reference silently falls back to a PyTorch path on ANY exception,
ops/modules/ms_deform_attn.py:116-121 -- deliberately not reproduced).
"""
import collections
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmsm_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "msm_hip.h")

_lib = None

_BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}

Header = collections.namedtuple("Header", "signatures params options abi_version opt_auto")


def _tokens(decl):
    """'const float*const* w' -> ['const', 'float', '*', 'const', '*', 'w']"""
    return decl.replace("*", " * ").split()


def _define(text, name):
    m = re.findall(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$" % name, text, flags=re.M)
    if len(m) != 1:
        raise ValueError(f"msm_hip.h: expected one integer `#define {name}`, found {len(m)}")
    return int(m[0])


def _options(body):
    """Names of the MSM_OPT_* enumerators (without prefix and COUNT); set_option passes the position as the key, so values
    must be the implicit 0, 1, 2, ..."""
    names = []
    items = [e.strip() for e in body.split(",")]
    for i, item in enumerate(items[:-1] if items[-1] == "" else items):
        m = re.fullmatch(r"MSM_OPT_(\w+)(?:\s*=\s*(.+))?", item, flags=re.S)
        if not m:
            raise ValueError(f"msm_hip.h: cannot read enumerator `{item}`")
        if m.group(2) is not None and (i, m.group(2).strip()) != (0, "0"):
            raise ValueError(f"msm_hip.h: enumerator `{item}` sets a value; option keys are positions, only `= 0` on the first is allowed")
        names.append(m.group(1))
    if not names or names[-1] != "COUNT" or "COUNT" in names[:-1] or len(set(names)) != len(names):
        raise ValueError("msm_hip.h: the MSM_OPT_* enum must hold distinct names and end with MSM_OPT_COUNT")
    return tuple(names[:-1])


def _prototype(stmt):
    m = re.fullmatch(r"([\w\s*]+?)\b(\w+)\s*\(([^(){}]*)\)", stmt)
    if not m:
        raise ValueError(f"msm_hip.h: not a function prototype: `{stmt}`")
    ret, name, plist = " ".join(_tokens(m.group(1))), m.group(2), m.group(3).strip()
    if ret != "const char *" and ret not in _BY_VALUE:
        raise ValueError(f"msm_hip.h: {name}: no ctypes rule for the return type `{ret}`")
    restype = _BY_VALUE.get(ret, ctypes.c_char_p)
    argtypes, names = [], []
    for p in ([] if plist in ("", "void") else plist.split(",")):
        *typ, pname = [t for t in _tokens(p) if t != "const"] or [""]
        typ = " ".join(typ)
        if not typ or not re.fullmatch(r"[A-Za-z_]\w*", pname):
            raise ValueError(f"msm_hip.h: {name}: parameter `{' '.join(p.split())}` needs a type and a plain name")
        if "*" not in typ and typ not in _BY_VALUE:
            raise ValueError(f"msm_hip.h: {name}: no ctypes rule for the by-value type `{typ}` of `{pname}`")
        argtypes.append(_BY_VALUE.get(typ, ctypes.c_void_p))
        names.append(pname)
    return name, (restype, argtypes), names


def parse_header(text):
    """The C ABI as include/msm_hip.h declares it: Header(signatures {name: (restype, [argtypes])} and params {name: [parameter
    names]} in declaration order, options (MSM_OPT_* names in enum order), abi_version, opt_auto).  Strict: every statement of
    the header must be understood, a ValueError names the one that is not."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    abi_version, opt_auto = _define(text, "MSM_ABI_VERSION"), _define(text, "MSM_OPT_AUTO")
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)
    text, wrappers = re.subn(r'\bextern\s*"C"\s*\{', " ", text)
    enums = re.findall(r"\benum\s*\{([^{}]*)\}\s*;", text)
    if len(enums) != 1:
        raise ValueError(f"msm_hip.h: expected one anonymous enum (MSM_OPT_*), found {len(enums)}")
    text = re.sub(r"\benum\s*\{[^{}]*\}\s*;", " ", text)
    *stmts, tail = text.split(";")
    if "".join(tail.split()) != "}" * wrappers:
        raise ValueError(f"msm_hip.h: unterminated statement at the end: `{' '.join(tail.split())}`")
    signatures, params = {}, {}
    for stmt in stmts:
        name, sig, names = _prototype(" ".join(stmt.split()))
        if name in signatures:
            raise ValueError(f"msm_hip.h: {name} is declared twice")
        signatures[name], params[name] = sig, names
    return Header(signatures, params, _options(enums[0]), abi_version, opt_auto)


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes bindings of libmsm_hip.so are read from it. "
                           "Keep include/ next to the package directory.")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


_HEADER = _load_header()            # once per process
_SIGNATURES = _HEADER.signatures
ABI_VERSION = _HEADER.abi_version   # lib() checks it against msm_abi_version() of the loaded library (a stale build)
# kernel-selection overrides, for tools/ and tests/ only: position in OPTIONS = value of MSM_OPT_<name>
OPTIONS = _HEADER.options
OPT_AUTO = _HEADER.opt_auto


def declared_symbols():
    """Function names declared in include/msm_hip.h (used by the symbol-export test)."""
    with open(HEADER_PATH) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(msm_[a-z0-9_]+)\s*\(", src)))


def lib():
    """Load libmsm_hip.so once; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the HIP hot path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.msm_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI {L.msm_abi_version()}, these bindings need {ABI_VERSION}: rebuild it")
        _lib = L
    return _lib


def set_option(name, value=OPT_AUTO):
    """msm_set_option(MSM_OPT_<name>, value); value OPT_AUTO restores the library's own choice.  Returns the old value."""
    key = OPTIONS.index(name)
    old = lib().msm_get_option(key)
    check(lib().msm_set_option(key, int(value)), "msm_set_option")
    if old != int(value):
        from ._plan import bump_plan_epoch
        bump_plan_epoch()          # captured graphs hold the kernels the old option selected: they re-capture (graphs.py)
    return old


class option:
    """``with option(name, value): ...`` (name: one of OPTIONS) -- scoped override, restored on exit."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


class CallTimer:
    """Measurement aid for bench.py: while active, every launch entry point of the library (``msm_*`` functions taking a
    stream) is bracketed by HIP events recorded on the stream it launches on (torch's current stream -- the one ops._stream()
    hands to the library).  ``durations()`` -> {entry point: [ms per call]} after a synchronize.  Eager launches only:
    events cannot time nodes inside a HIP-graph replay."""

    def __init__(self):
        self.records = []
        self._saved = {}

    @staticmethod
    def timed_entry_points():
        """The launch entry points: the functions whose last parameter is the stream."""
        return [name for name, names in _HEADER.params.items() if names[-1:] == ["stream"]]

    def __enter__(self):
        import torch
        L = lib()
        for name in self.timed_entry_points():
            fn = getattr(L, name)
            self._saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = _fn(*a)
                e1.record()
                self.records.append((_name, e0, e1))
                return rc

            setattr(L, name, wrapped)
        return self

    def __exit__(self, *exc):
        L = lib()
        for name, fn in self._saved.items():
            setattr(L, name, fn)
        self._saved = {}
        return False

    def durations(self):
        out = {}
        for name, e0, e1 in self.records:
            out.setdefault(name, []).append(e0.elapsed_time(e1))
        return out


def check(rc, what):
    if rc != 0:
        msg = lib().msm_last_error_string()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
