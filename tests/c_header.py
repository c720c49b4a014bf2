"""A ctypes binding of ``libscratchpad_hip.so`` derived from ``include/scratchpad_hip.h`` alone.

This is how an integrator binds the library: from the header, not from
``scratchpad_amd/_native.py``.  Every ``SP_API`` prototype is parsed into (name, return ctype,
[(parameter name, ctype)]); ``bind()`` opens the library as a handle of its own with these argtypes and
``call()`` passes keyword arguments in the header's parameter order, so a test spells out every
parameter by the name the header gives it.  A plain module (not a conftest): the tests import it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scratchpad_hip.h")

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_POINTEES = ("void", "int32_t", "int64_t", "float", "int")      # T* -> c_void_p for these T


def _text() -> str:
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def ctype_of(decl: str):
    """ctypes type of a C type as the header spells it; ValueError for a type the map does not know."""
    t = " ".join(decl.replace("*", " * ").split())
    if t == "const char *":
        return ctypes.c_char_p
    if t in _SCALARS:
        return _SCALARS[t]
    if t in ("void * *", "void * const *"):
        return ctypes.c_void_p
    base = t[len("const "):] if t.startswith("const ") else t
    if base.endswith(" *") and base[:-2] in _POINTEES:
        return ctypes.c_void_p
    raise ValueError(f"C type {decl!r} is not in the header binding's type map")


def _split_param(p: str):
    m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p)
    if not m:
        raise ValueError(f"cannot read the parameter {p!r}")
    return m.group(2), m.group(1).strip()


def prototypes() -> dict:
    """name -> (return ctype, [(parameter name, ctype)]) for every SP_API prototype, in header order."""
    out = {}
    for m in re.finditer(r"\bSP_API\s+([^;{}()]*?)\b(sp_\w+)\s*\(([^)]*)\)\s*;", _text()):
        ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
        args = []
        if params not in ("", "void"):
            for p in params.split(","):
                pname, ptype = _split_param(p)
                args.append((pname, ctype_of(ptype)))
        out[name] = (ctype_of(ret), args)
    return out


def abi_version() -> int:
    return int(re.search(r"#define\s+SP_ABI_VERSION\s+(\d+)", _text()).group(1))


def enum_values(type_name: str) -> dict:
    """{enumerator: value} of `typedef enum { ... } type_name;`."""
    m = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*" + re.escape(type_name) + r"\s*;", _text())
    if not m:
        raise ValueError(f"no enum {type_name} in the header")
    return {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", m.group(1))}


def bind(path: str) -> ctypes.CDLL:
    """The library as a CDLL object of its own (its function objects are not _native's) with the header's types."""
    lib = ctypes.CDLL(path)
    lib.sp_prototypes = prototypes()
    for name, (res, args) in lib.sp_prototypes.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = [t for _, t in args]
    return lib


def _value(v):
    return v.data_ptr() if hasattr(v, "data_ptr") else v


def call(lib: ctypes.CDLL, name: str, **kwargs):
    """lib.name(...) with the arguments given by their header names (tensors by their device pointer).
    TypeError on a missing or an unknown name."""
    params = [p for p, _ in lib.sp_prototypes[name][1]]
    unknown = sorted(set(kwargs) - set(params))
    missing = [p for p in params if p not in kwargs]
    if unknown or missing:
        raise TypeError(f"{name}: unknown {unknown}, missing {missing}")
    return getattr(lib, name)(*[_value(kwargs[p]) for p in params])
