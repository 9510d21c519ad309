"""The ctypes side of the C ABI, derived from include/occdepth_amd.h at import: the header is the only definition.

CONSTANTS   {"OCCD_MAX_VIEWS": 4, ...}                     every `#define NAME integer`
STRUCTS     {"occd_conv3d_args": <ctypes.Structure>, ...}   every `typedef struct T {...} T;` (the field `in` is `inp`)
EXPORTS     {"occd_conv3d_fwd": (restype, [argtypes]), ...} every function declaration
ABI_VERSION OCCD_ABI_VERSION

parse() understands the subset of C the header uses -- block comments, `#define NAME integer`, structs of plain
declarators (`*`, `const`, `[N]` with literal or OCCD_* extents, several declarators per base type, structs by value) and
function declarations -- and RAISES on everything else: a construct that were skipped would be a hole in the binding.
Pointer arguments: to a parsed struct -> POINTER(Struct); `const char*` -> c_char_p; `void**` -> POINTER(c_void_p); every
other one -> c_void_p (callers pass tensor.data_ptr() integers or ctypes.byref(...)).  Pointer FIELDS are all c_void_p:
a field holds a raw address (a.chunks = table.data_ptr()).
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "occdepth_amd.h")
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double,
           "char": ctypes.c_char, "void": None}
_IDENT = re.compile(r"[A-Za-z_]\w*$")


class HeaderError(ValueError):
    """The header uses C outside the parsed subset."""


def _split(toks, sep, what):
    """toks = item sep item sep ... -> the items; with sep ';' the last item must be terminated as well."""
    items, cur = [], []
    for t in toks:
        if t == sep:
            items.append(cur)
            cur = []
        else:
            cur.append(t)
    if sep == ",":
        items.append(cur)
    elif cur:
        raise HeaderError(f"{what}: unterminated `{' '.join(cur)}`")
    return items


def _find(toks, t, i):
    return toks.index(t, i) if t in toks[i:] else len(toks)


def _declarator(toks, base, consts, structs, field=False):
    """[const] base [const] {* | const} [name] {[extent]} (the base is inherited when `base` is given) ->
    (base, ctype or None for plain void, name or None).  field: a struct member, whose pointers are raw addresses."""
    text = " ".join(toks)
    toks = list(toks)
    if base is None:
        while toks and toks[0] == "const":
            toks.pop(0)
        base = toks.pop(0) if toks else None
        if base not in SCALARS and base not in structs:
            raise HeaderError(f"unknown type in `{text}`")
    stars = 0
    while toks and toks[0] in ("*", "const"):
        stars += toks.pop(0) == "*"
    name = toks.pop(0) if toks and _IDENT.match(toks[0]) and toks[0] not in SCALARS and toks[0] != "const" else None
    extents = []
    while len(toks) >= 3 and toks[0] == "[" and toks[2] == "]":
        ext = consts.get(toks[1]) if _IDENT.match(toks[1]) else int(toks[1], 0)
        if ext is None:
            raise HeaderError(f"array extent {toks[1]} of `{text}` is not an integer #define")
        extents.append(ext)
        del toks[:3]
    if toks:
        raise HeaderError(f"cannot parse `{' '.join(toks)}` in `{text}`")
    if stars == 0:
        ctype = structs.get(base) or SCALARS[base]
    elif field:
        ctype = ctypes.c_void_p
    elif stars == 1 and base in structs:
        ctype = ctypes.POINTER(structs[base])
    elif stars == 1 and base == "char":
        ctype = ctypes.c_char_p
    elif stars == 2 and base == "void":
        ctype = ctypes.POINTER(ctypes.c_void_p)
    else:
        ctype = ctypes.c_void_p
    if extents and ctype is None:
        raise HeaderError(f"array of void in `{text}`")
    for n in reversed(extents):
        ctype = ctype * n
    return base, ctype, name


def parse(text):
    """Header text -> (constants, structs, exports)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\b.*?#endif", " ", text, flags=re.S)      # the extern "C" brackets
    consts, structs, exports, code = {}, {}, {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        word = line.split()
        if word[0] == "#define" and len(word) >= 3 and _IDENT.match(word[1]):
            try:
                consts[word[1]] = int("".join(word[2:]).strip("()"), 0)
            except ValueError:
                consts[word[1]] = None            # an error only where it is used as an array extent
        elif not (word[0] in ("#define", "#include", "#ifndef") and len(word) == 2 or word == ["#endif"]):
            raise HeaderError(f"unsupported directive `{line.strip()}`")
    code = "\n".join(code)
    token = r"\w+|[*\[\](){},;]"
    junk = re.sub(token + r"|\s+", "", code)
    if junk:
        raise HeaderError(f"unsupported characters {junk[:20]!r}")
    toks = re.findall(token, code)                # whole words: `scale_const` is not `scale_` + `const`
    i = 0
    while i < len(toks):
        if toks[i] == "typedef":                  # typedef struct T { fields } T ;
            close = _find(toks, "}", i)
            tag = toks[i + 2] if i + 2 < len(toks) else ""
            body = toks[i + 4:close]
            if toks[i + 1:i + 4] != ["struct", tag, "{"] or toks[close + 1:close + 3] != [tag, ";"] \
                    or not _IDENT.match(tag) or tag in structs:
                raise HeaderError(f"unsupported typedef near `{' '.join(toks[i:i + 8])}`")
            if set(body) & set("(){}"):
                raise HeaderError(f"{tag}: function pointers and nested definitions are not supported")
            fields = []
            for decl in _split(body, ";", tag):
                base = None
                for d in _split(decl, ",", tag):
                    base, ctype, name = _declarator(d, base, consts, structs, field=True)
                    if ctype is None or name is None:
                        raise HeaderError(f"{tag}: `{' '.join(decl)}` is not a field")
                    fields.append(("inp" if name == "in" else name, ctype))
            structs[tag] = type(tag, (ctypes.Structure,), {"_fields_": fields})
            i = close + 3
            continue
        end = _find(toks, ";", i)                 # restype name ( void | parameters ) ;
        stmt = toks[i:end]
        lp = stmt.index("(") if "(" in stmt else 0
        params = stmt[lp + 1:-1]
        if end == len(toks) or lp == 0 or stmt[-1] != ")" or set(stmt[:lp] + params) & set("(){}[]"):
            raise HeaderError(f"unsupported declaration `{' '.join(stmt[:12])}`")
        _, restype, name = _declarator(stmt[:lp], None, consts, structs)
        if name is None or name in exports:
            raise HeaderError(f"unnamed or repeated function in `{' '.join(stmt[:12])}`")
        args = [] if params == ["void"] else [_declarator(p, None, consts, structs)[1] for p in _split(params, ",", name)]
        if None in args:
            raise HeaderError(f"{name}: a parameter of type void")
        exports[name] = (restype, args)
        i = end + 1
    return consts, structs, exports


if not os.path.exists(HEADER):
    raise RuntimeError(f"{HEADER} is missing: the ctypes binding of libocc_hip.so is derived from it "
                       "(the header is the only definition of the ABI)")
with open(HEADER) as _f:
    CONSTANTS, STRUCTS, EXPORTS = parse(_f.read())
ABI_VERSION = CONSTANTS["OCCD_ABI_VERSION"]
