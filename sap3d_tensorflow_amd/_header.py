"""Reads include/p3d_hip.h into what ctypes needs: the header is the one place where the boundary is written down.

parse(text) accepts the grammar the header's "Conventions" comment states and nothing more; whatever it cannot place
raises HeaderError with the offending text.  Nothing is guessed and nothing is skipped silently."""
import collections
import ctypes as C
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p3d_hip.h")

# functions {name: (restype, argtypes)}, structs {typedef name: Structure subclass}, constants {NAME: int}
Header = collections.namedtuple("Header", "functions structs constants")


class HeaderError(ValueError):
    pass


SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "char": C.c_char, "unsigned char": C.c_ubyte,
           "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
OPAQUE = ("void", "p3d_handle")          # known by address only: T* is c_void_p
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
# [const] base [* [const] [*]] [name] [[N]]
_DECL = re.compile(r"(?:const )?(unsigned char|\w+)\b ?((?:\* ?(?:const\b ?)?)*)(\w+)?(?: ?\[(\d+)\])?")
_DIRECTIVES = re.compile(r"#\s*(?:include\s*<\w+\.h>|ifndef\s+\w+|ifdef\s+__cplusplus|endif)")


def class_name(name):
    """p3d_video_temporal -> P3dVideoTemporal"""
    return "".join(p.capitalize() for p in name.split("_"))


def _statements(text, constants):
    """The header's statements up to their `;`, white space squeezed.  Block comments go; preprocessor lines go after
    `#define NAME <integer>` has been read; what sits between `#ifdef __cplusplus` and its `#endif` is not C and goes too."""
    text, code, cxx = re.sub(r"/\*.*?\*/", " ", text, flags=re.S), [], False
    for line in text.splitlines():
        s = line.strip()
        if not s.startswith("#"):
            if not cxx:
                code.append(line)
            continue
        m = re.fullmatch(r"#\s*define\s+(\w+)\s*(.*)", s)
        if m:                                          # any other body (the include guard, an expression) is not a constant
            if re.fullmatch(_INT, m.group(2)):
                constants[m.group(1)] = int(m.group(2), 0)
        elif not _DIRECTIVES.fullmatch(s):
            raise HeaderError("preprocessor line outside the grammar: %r" % s)
        elif not s.endswith(".h>"):                    # an #endif ends the C++ part, if one is open; nothing nests inside it
            cxx = s.endswith("__cplusplus")
    text, end = "\n".join(code), 0
    for m in re.finditer(r"((?:[^;{}]|\{[^{}]*\})*);", text):
        if m.start() != end:
            break
        end = m.end()
        yield " ".join(m.group(1).split())
    if text[end:].strip():
        raise HeaderError("not a statement: %r" % " ".join(text[end:].split())[:120])


def _ctype(base, stars, structs, where):
    """The type rule: scalars are their ctypes twins, p3d_handle* and void* are c_void_p, char* is c_char_p, any other T* is
    POINTER(T), and a second level of pointer is POINTER of the first."""
    if stars > 2:
        raise HeaderError("more than two levels of pointer in %r" % where)
    if stars == 0:
        if base in SCALARS:
            return SCALARS[base]
        if base in structs:
            return structs[base]
        raise HeaderError("unknown type %r in %r (the closed set of scalars, or a struct defined above its use)" % (base, where))
    if stars == 1 and base in OPAQUE:
        return C.c_void_p
    if stars == 1 and base == "char":
        return C.c_char_p
    return C.POINTER(_ctype(base, stars - 1, structs, where))


def _declarator(text, structs, where):
    """(name, ctype, array length or None) of `[const] T [*[const][*]] name[[N]]`."""
    m = _DECL.fullmatch(text)
    if not m or not m.group(3):
        raise HeaderError("not a declaration: %r in %r" % (text, where))
    base, stars, name, n = m.groups()
    return name, _ctype(base, stars.count("*"), structs, where), n and int(n)


def _struct(name, body, structs):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        fname, t, n = _declarator(first, structs, decl)
        if more and "*" in first:
            raise HeaderError("several declarators after a pointer: %r" % decl)
        fields.append((fname, t * n if n else t))
        for d in more:                                  # `int ld, off;`: the base type again
            m = re.fullmatch(r"(\w+)(?: ?\[(\d+)\])?", d)
            if not m:
                raise HeaderError("not a declarator: %r in %r" % (d, decl))
            fields.append((m.group(1), t * int(m.group(2)) if m.group(2) else t))
    return type(class_name(name), (C.Structure,), {"_fields_": fields, "__doc__": "%s of include/p3d_hip.h" % name})


def parse(text):
    functions, structs, constants = {}, {}, {}
    for st in _statements(text, constants):
        m = re.fullmatch(r"enum ?\{(.*)\}", st)
        if m:
            for e in m.group(1).split(","):
                em = re.fullmatch(r"\s*(\w+) ?= ?(%s)\s*" % _INT, e)
                if not em:
                    raise HeaderError("enumerator without an explicit integer value: %r in %r" % (e.strip(), st))
                constants[em.group(1)] = int(em.group(2), 0)
            continue
        m = re.fullmatch(r"typedef struct ?(\w+)? ?\{(.*)\} ?(\w+)", st)
        if m:
            structs[m.group(3)] = _struct(m.group(3), m.group(2), structs)
            continue
        if st == "typedef struct p3d_handle p3d_handle":
            continue
        m = re.fullmatch(r"([\w *]+?) ?\b(\w+) ?\(([^()]*)\)", st)
        if not m:
            raise HeaderError("cannot classify the statement %r" % st)
        ret, name, params = m.groups()
        res = None if ret == "void" else _declarator(ret + " _", structs, st)[1]
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            _, t, n = _declarator(p.strip(), structs, st)
            args.append(t if n is None else C.POINTER(t))          # a parameter `T name[N]` is a T*
        functions[name] = (res, args)
    return Header(functions, structs, constants)


def read():
    with open(PATH) as f:
        return parse(f.read())
