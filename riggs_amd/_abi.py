"""The C ABI as ctypes objects, read from include/riggs_hip.h — the one place it is written down.

``FUNCTIONS``: name -> (restype, [argtypes]); ``STRUCTS``: C name -> ``ctypes.Structure`` with the header's field names;
``CONSTANTS``: every enumerator and every ``#define RIGGS_* <integer>``.  The header is plain C in a narrow style (no function
pointers, no bit fields, no nested braces), which is all this reads; a declaration outside that style raises with its line — it is
never skipped.  tests/test_capi_cpu.py has the compiler check every signature and every struct layout derived here."""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "riggs_hip.h")

FUNCTIONS, STRUCTS, CONSTANTS = {}, {}, {}
_TYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
          "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}  # by value; typedefs and structs join as they are read


class HeaderError(ValueError):
    pass


def _ctype(spec, line):
    """``const float* const*`` -> c_void_p, ``int32_t`` -> c_int32, ``const riggs_gate*`` -> POINTER(riggs_gate), ..."""
    words = [w for w in re.findall(r"\w+", spec) if w not in ("const", "struct")]
    stars = spec.count("*")
    if len(words) != 1 or re.search(r"[^\w\s*]", spec):
        raise HeaderError("%s:%d: cannot read the type '%s'" % (HEADER, line, spec.strip()))
    base = words[0]
    if stars == 0:
        if base not in _TYPES:
            raise HeaderError("%s:%d: cannot read the type '%s': nothing above declares it" % (HEADER, line, base))
        return _TYPES[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in STRUCTS:
        return C.POINTER(STRUCTS[base])
    return C.c_void_p


def _declarator(text, line):
    """``const float* w[8]`` -> ('const float* ', 'w', 8); the bound is a literal or one of the header's constants."""
    m = re.fullmatch(r"\s*(.*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", text, flags=re.S)
    if not m or (m.group(3) and not (m.group(3).isdigit() or m.group(3) in CONSTANTS)):
        raise HeaderError("%s:%d: cannot read the declarator '%s'" % (HEADER, line, " ".join(text.split())))
    bound = m.group(3)
    return m.group(1), m.group(2), None if bound is None else CONSTANTS[bound] if bound in CONSTANTS else int(bound)


def _struct(name, body, line):
    fields = []
    for decl in filter(str.strip, body.split(";")):          # "const float *W_rot, *b_rot": one base type, its stars per name
        parts = [_declarator(d, line) for d in decl.split(",")]
        base = parts[0][0].replace("*", " ")
        for i, (spec, field, bound) in enumerate(parts):
            if i and spec.strip(" \t\n*"):
                raise HeaderError("%s:%d: cannot read the field '%s' of %s" % (HEADER, line, field, name))
            t = _ctype(base + "*" * spec.count("*"), line)
            fields.append((field, t if bound is None else t * bound))
    STRUCTS[name] = _TYPES[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": "%s (include/riggs_hip.h)." % name})


def _enum(body, line):
    value = -1
    for item in filter(str.strip, body.split(",")):
        m = re.fullmatch(r"\s*(\w+)\s*(?:=\s*(-?\w+))?\s*", item)
        try:
            value = value + 1 if m.group(2) is None else int(m.group(2), 0)
        except (AttributeError, ValueError):
            raise HeaderError("%s:%d: cannot read the enumerator '%s'" % (HEADER, line, item.strip())) from None
        CONSTANTS[m.group(1)] = value


def _read():
    keep_lines = lambda m: "\n" * m.group(0).count("\n")     # whatever is cut out leaves its line breaks: positions name lines
    txt = re.sub(r"/\*.*?\*/", keep_lines, open(HEADER).read(), flags=re.S)
    txt = re.sub(r"#ifdef __cplusplus\n.*?#endif", keep_lines, txt, flags=re.S)
    for m in re.finditer(r"^[ \t]*#define[ \t]+(RIGGS_\w+)[ \t]+(\S.*?)[ \t]*$", txt, flags=re.M):
        try:
            CONSTANTS[m.group(1)] = int(m.group(2), 0)
        except ValueError:
            raise HeaderError("%s:%d: #define %s is not an integer" % (HEADER, txt.count("\n", 0, m.start()) + 1, m.group(1))) from None
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)

    def lift(m):
        line = txt.count("\n", 0, m.start()) + 1
        if m.group(1) == "enum":
            _enum(m.group(3), line)
        else:
            _struct(m.group(2), m.group(3), line)
        return keep_lines(m)
    txt = re.sub(r"(?:typedef\s+)?\b(struct|enum)\s*(\w*)\s*\{([^{}]*)\}\s*\w*\s*;", lift, txt)
    pos = 0
    for decl in txt.split(";"):
        line = txt.count("\n", 0, pos + len(decl) - len(decl.lstrip())) + 1
        pos += len(decl) + 1
        if not decl.strip():
            continue
        fn = re.fullmatch(r"\s*(.*?)\b(riggs_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if decl.split()[0] == "typedef":                     # typedef void* riggs_stream
            spec, name, _ = _declarator(decl.split(None, 1)[1], line)
            _TYPES[name] = _ctype(spec, line)
        elif fn and "(" not in fn.group(3):
            args = [] if fn.group(3).strip() == "void" else [_declarator(a, line)[0] for a in fn.group(3).split(",")]
            FUNCTIONS[fn.group(2)] = (_ctype(fn.group(1), line), [_ctype(a, line) for a in args])
        else:
            raise HeaderError("%s:%d: cannot read the declaration '%s'" % (HEADER, line, " ".join(decl.split())))


_read()
