"""The C boundary of libmcedm_hip.so, read from include/mcedm_hip.h: the one source of the binding's constants, struct layouts
and signatures (lib.py applies them to the loaded library; nothing here imports torch).

CONSTS   every ``#define MCEDM_* <integer expression>`` and every mcedm_status enumerator: name -> int
STRUCTS  every ``typedef struct {...} name;``: name -> ctypes.Structure class with the header's fields in the header's order
PROTOS   every prototype: name -> (restype, argtypes)
DECLS    the same prototypes as C text without the parameter names: name -> (return type, [argument types]); what the tests
         hand to a C compiler next to PROTOS

Argument types: a pointer to one of the header's ``*_desc`` structs (the host-side descriptions) is POINTER(its class), ``char*``
is c_char_p and every other pointer (opaque plans, float*, size_t*, const float* const*, int64_t shape[4], the mcedm_coef tables
in device memory) is c_void_p, which takes an int, None, byref(...) and a ctypes array alike; scalars map by name.  A pointer FIELD of a struct keeps its target type (POINTER(c_float), POINTER(c_double)).  The parser
knows the header's own constructs and no more: anything else raises ValueError with the file and line instead of being skipped.
"""
import ctypes as C
import os
import re

HEADER = os.environ.get("MCEDM_HEADER") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "include", "mcedm_hip.h")   # MCEDM_HEADER: A/B builds, with MCEDM_LIB
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
CONSTS, STRUCTS, PROTOS, DECLS = {}, {}, {}, {}


def _int(expr: str) -> int:
    """An integer expression of literals, earlier constants, + - * and parentheses."""
    if not re.fullmatch(r"[\w\s()+*-]+", expr):
        raise ValueError(expr)
    return int(eval(expr, {"__builtins__": {}}, CONSTS))


def _decl(d: str):
    """'const float* x' -> ('const float*', 'x', None); 'int64_t shape[4]' -> ('int64_t', 'shape', '[4]')."""
    return re.fullmatch(r"(.*[\w*]) ?\b(\w+)(\[\w+\])?", d.strip()).groups()


def _ctype(t: str, field: bool = False):
    """The ctypes class of the C type ``t`` (no declarator name) as an argument or return type, or as a struct field."""
    base, ptr = re.fullmatch(r"(?:const )?([\w ]+?) ?((?:\* ?(?:const ?)?)+|\[\w+\])?", t).groups()
    if not ptr:
        return _SCALARS[base]
    if ptr.strip() == "*":
        if base in STRUCTS and base.endswith("_desc"):     # (mcedm_coef rows live in device memory: an address, like float*)
            return C.POINTER(STRUCTS[base])
        if base == "char":
            return C.c_char_p
        if field:
            return C.POINTER(_SCALARS[base])
    return C.c_void_p


def _statement(s: str) -> None:
    if m := re.fullmatch(r"typedef enum \{(.*)\} \w+", s):
        for item in m.group(1).split(","):
            name, value = item.split("=")
            CONSTS[name.strip()] = _int(value)
    elif m := re.fullmatch(r"typedef struct (?:\w+ )?\{(.*)\} (\w+)", s):
        fields = []
        for line in filter(None, map(str.strip, m.group(1).split(";"))):
            first, *more = line.split(",")                 # `double sigma_min, sigma_max, rho`: one type, declarators in order
            t, name, arr = _decl(first)
            for name, arr in [(name, arr)] + [re.fullmatch(r"(\w+)(\[\w+\])?", x.strip()).groups() for x in more]:
                fields.append((name, _ctype(t, True) * _int(arr[1:-1]) if arr else _ctype(t, True)))
        STRUCTS[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
    elif re.fullmatch(r"typedef struct (\w+) \1", s):      # an opaque handle: its pointers are c_void_p like any other
        pass
    elif m := re.fullmatch(r"([\w ]+?\*?) ?(mcedm_\w+) ?\((.*)\)", s):
        ret, name, args = m.groups()
        texts = [] if args == "void" else [t + (arr or "") for t, _, arr in map(_decl, args.split(","))]
        PROTOS[name] = (None if ret == "void" else _ctype(ret), [_ctype(t) for t in texts])
        DECLS[name] = (ret, texts)
    else:
        raise ValueError(s)


def _parse(path: str) -> None:
    def fail(no, text, err):
        raise ValueError(f"{path}:{no}: not a construct this parser knows: {' '.join(text.split())!r}") from err

    with open(path) as f:                                   # comments out, line numbers kept
        src = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), f.read(), flags=re.S)
    body, cxx = [], False
    for no, line in enumerate(src.split("\n"), 1):
        if not line.lstrip().startswith("#"):
            body.append("" if cxx else line)               # C++-only lines (extern "C") are not part of the C boundary
            continue
        body.append("")
        try:
            if m := re.fullmatch(r"\s*#define (\w+)(?:\s+(\S.*?))?\s*", line):
                if m.group(2):                             # (a define without a value is the include guard)
                    CONSTS[m.group(1)] = _int(m.group(2))
            elif line.split() == ["#ifdef", "__cplusplus"] or line.split() == ["#endif"]:
                cxx = line.split()[0] == "#ifdef"
            elif line.split()[0] not in ("#include", "#ifndef"):
                raise ValueError(line)
        except Exception as e:
            fail(no, line, e)
    text = "\n".join(body)
    for m in re.finditer(r"((?:[^;{}]|\{[^{}]*\})+);|\S", text):   # a statement up to its `;`, or a character that is in none
        try:
            _statement(" ".join((m.group(1) or "").split()))
        except Exception as e:
            fail(text.count("\n", 0, m.end() - len(m.group().lstrip())) + 1, m.group(), e)


_parse(HEADER)
