"""A small parser of the C headers under include/, for tests/test_abi_and_host.py: every prototype's return and parameter
types and every `typedef struct ctd_*`, read from the text that is left after comments and preprocessor lines are gone.
It knows the C that these headers use and nothing more; whatever it does not recognise raises, so that a new kind of
declaration is looked at instead of skipped."""
import re

SCALARS = ("int", "long", "float", "double", "size_t", "int32_t", "int64_t", "uint64_t")

_IDENT = r"[A-Za-z_]\w*"


def _type_and_name(decl, what):
    """'const float* in0' -> ('float*', 'in0'); 'int' -> ('int', None).  A pointer is its pointee's words and a '*', a
    scalar is one of SCALARS; `const` is dropped."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        star = len(words) - 1 - words[::-1].index("*")
        ctype, rest = " ".join(words[:star]).replace(" *", "*") + "*", words[star + 1:]
    else:
        ctype, rest = words[0] if words else "", words[1:]
        if ctype not in SCALARS:
            raise ValueError("%s: unknown type word in '%s'" % (what, decl.strip()))
    if len(rest) > 1 or not all(re.fullmatch(_IDENT, w) for w in rest):
        raise ValueError("%s: cannot read '%s'" % (what, decl.strip()))
    return ctype, (rest[0] if rest else None)


def parse_header(path):
    """-> (functions, structs): functions[name] = (return type, [parameter types]) with 'void' and 'char*' as further
    return types, structs[name] = [(field, type), ...] in order, an array field typed like 'float[5]'."""
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*", " ", src, flags=re.M)
    src = src.replace('extern "C" {', " ")
    src = re.sub(r"\benum\s+%s\s*\{[^{}]*\}\s*;" % _IDENT, " ", src)
    structs = {}

    def struct(m):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise ValueError("%s: typedef struct %s is named %s" % (path, name, m.group(3)))
        for line in filter(None, (s.strip() for s in m.group(2).split(";"))):
            first, *more = line.split(",")
            base, field = _type_and_name(re.sub(r"\[\d+\]", "", first), name)
            base = base.rstrip("*")
            for d in [first[re.search(r"\b%s\b" % base, first).end():]] + more:
                dm = re.fullmatch(r"\s*(\*?)\s*(%s)\s*(\[\d+\])?\s*" % _IDENT, d)
                if not dm:
                    raise ValueError("%s: cannot read field '%s' of %s" % (path, line, name))
                fields.append((dm.group(2), base + dm.group(1) + (dm.group(3) or "")))
        structs[name] = fields
        return " "
    src = re.sub(r"typedef\s+struct\s+(ctd_\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, src)
    functions = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        if stmt == "}":                                              # the end of extern "C"
            continue
        m = re.fullmatch(r"([\w\s\*]+?)\s*\b(ctd_\w+)\s*\(([^()]*)\)", stmt)
        if not m or m.group(2) in functions:
            raise ValueError("%s: cannot read '%s'" % (path, stmt))
        name, params = m.group(2), m.group(3).strip()
        ret = " ".join(w for w in m.group(1).replace("*", " * ").split() if w != "const").replace(" *", "*")
        if ret not in SCALARS + ("void", "char*"):
            raise ValueError("%s: unknown return type '%s'" % (name, m.group(1)))
        functions[name] = (ret, [] if params in ("", "void") else
                           [_type_and_name(p, "%s, parameter %d" % (name, i))[0] for i, p in enumerate(params.split(","))])
    return functions, structs
