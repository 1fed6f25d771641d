#!/usr/bin/env python3
"""Parser of include/boojum_hip.h: ONE language-neutral description of the C ABI, which tools/gen_rust_bindings.py turns into
rust/boojum_hip_sys.rs and tools/gen_py_abi.py into era_boojum_amd/_abi.py.

A declaration is (name, CType).  CType records the base C type as the header spells it ("unsigned", "uint64_t", "bj_ctx", ...),
per pointer level — innermost first — whether the thing pointed to is const, the extent of an array FIELD (None otherwise) and,
for a function-pointer declarator written in place (the callbacks of bj_comm), its signature (return CType, [declarations]).
A function-pointer TYPEDEF used by name is a CType whose base is that name; the signatures are in `fn_types`.  An array
PARAMETER has already decayed to a pointer (C11 6.7.6.3p7), an array field keeps its extent.

parse_header() returns a dict of
    defines      [(name, value as written, without a U suffix)]
    enums        {enum name: [(enumerator, value)]}          named enums only
    enum_consts  [(enumerator, value)]                       every enumerator, anonymous enums included, in header order
    opaque       [struct names that are only forward-declared]
    structs      [(name, [field declarations])]
    fn_types     [(typedef name, (return CType, [parameter declarations]))]
    funcs        [(name, return CType, [parameter declarations])]
"""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "boojum_hip.h")
DIAG_HEADER = os.path.join(ROOT, "include", "boojum_hip_diag.h")   # diagnostics beside the ABI: its own generated modules

CType = collections.namedtuple("CType", "base consts extent fn")
CType.__new__.__defaults__ = ((), None, None)


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def parse_type(ctype):
    """C type without a declarator name -> CType.  `const T *const *`: the constness of the POINTEE is what a pointer level
    records, so a const that follows the last `*` (a const pointer variable) is dropped."""
    consts, cur_const, name_parts = [], False, []
    for tok in ctype.replace("*", " * ").split():
        if tok == "const":
            cur_const = True
        elif tok == "*":
            consts.append(cur_const)
            cur_const = False
        else:
            name_parts.append(tok)
    assert name_parts, "no base type in %r" % ctype
    return CType(" ".join(name_parts), tuple(consts))


def split_params(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch == "(":
            depth += 1
        if ch == ")":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def parse_param(p, decay=False):
    """'const uint64_t *d_in' -> ("d_in", CType).  `decay`: the declaration is a FUNCTION PARAMETER, where C adjusts an array type
    `T name[N]` to the pointer `T *name` — a binding that passed N elements by value would push them where the callee expects
    one address; struct fields keep their arrays."""
    m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)(\[(\d*)\])?$", p.strip())
    ctype, name, brackets, arr = m.groups()
    if brackets and decay:
        return name, parse_type(ctype.rstrip() + " *")
    t = parse_type(ctype)
    if brackets:
        assert arr, "an array field needs its extent: %r" % p
        t = t._replace(extent=int(arr))
    return name, t


def parse_fn_pointer(decl):
    """'int (*name)(void *user, size_t bytes)' -> (name, (return CType, [parameter declarations]))."""
    m = re.match(r"^(.*?)\(\s*\*\s*([A-Za-z_][A-Za-z0-9_]*)\s*\)\s*\((.*)\)$", decl.strip(), flags=re.S)
    ret, name, params = m.groups()
    return name, (parse_type(ret), [parse_param(p, decay=True) for p in split_params(params)])


def parse_header(path=HEADER):
    src = strip_comments(open(path).read())
    defines = [(m.group(1), m.group(2)) for m in re.finditer(r"^#define\s+(BJ_[A-Z0-9_]+)\s+(\d+|0[xX][0-9a-fA-F]+)[uU]?\s*$", src, flags=re.M)]
    enums, enum_consts = {}, []
    for m in re.finditer(r"(typedef\s+)?enum\s*([A-Za-z_0-9]*)\s*\{(.*?)\}\s*([A-Za-z_0-9]*)\s*;", src, flags=re.S):
        name = m.group(4) or m.group(2)
        items = []
        nxt = 0
        for it in m.group(3).split(","):
            it = it.strip()
            if not it:
                continue
            if "=" in it:
                k, v = (x.strip() for x in it.split("="))
                nxt = int(v, 0)
            else:
                k = it
            items.append((k, nxt))
            nxt += 1
        if name:
            enums[name] = items
        enum_consts += items
    opaque = re.findall(r"typedef\s+struct\s+([A-Za-z_0-9]+)\s+\1\s*;", src)
    structs = []
    for m in re.finditer(r"typedef\s+struct\s+([A-Za-z_0-9]+)\s*\{(.*?)\}\s*\1\s*;", src, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            if re.search(r"\(\s*\*", decl):
                name, sig = parse_fn_pointer(decl)
                fields.append((name, CType("", fn=sig)))
                continue
            # `unsigned rank, world` style lists
            first = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*(\[\d+\])?)((\s*,\s*[A-Za-z_][A-Za-z0-9_]*)*)$", decl)
            ctype = first.group(1)
            names = [first.group(2)] + [x.strip() for x in first.group(4).split(",") if x.strip()]
            for nm in names:
                fields.append(parse_param(ctype + " " + nm))
        structs.append((m.group(1), fields))
    fn_typedef = r"typedef\s+([A-Za-z_][A-Za-z0-9_ \*]*?)\(\s*\*\s*(bj_[A-Za-z0-9_]+)\s*\)\s*\(([^;]*?)\)\s*;"
    fn_types = [parse_fn_pointer("%s (*%s)(%s)" % (m.group(1), m.group(2), " ".join(m.group(3).split())))
                for m in re.finditer(fn_typedef, src, flags=re.S)]
    body = re.sub(fn_typedef, " ", src, flags=re.S)
    body = re.sub(r"typedef\s+struct\s+[A-Za-z_0-9]+\s*\{.*?\}\s*[A-Za-z_0-9]+\s*;", " ", body, flags=re.S)
    body = re.sub(r"(typedef\s+)?enum\s*[A-Za-z_0-9]*\s*\{.*?\}\s*[A-Za-z_0-9]*\s*;", " ", body, flags=re.S)
    body = re.sub(r"^#.*$", " ", body, flags=re.M)
    body = body.replace('extern "C" {', " ").replace("}", " ")
    funcs = []
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(bj_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", body, flags=re.S):
        ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        if ret.startswith("typedef"):
            continue
        ps = [] if params in ("void", "") else [parse_param(p, decay=True) for p in split_params(params)]
        funcs.append((name, parse_type(ret), ps))
    return dict(defines=defines, enums=enums, enum_consts=enum_consts, opaque=opaque, structs=structs, funcs=funcs, fn_types=fn_types)


def write_if_changed(path, txt):
    """Generated sources are committed: the file is rewritten only when its text changes (a build must leave a clean tree)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if not os.path.exists(path) or open(path).read() != txt:
        with open(path, "w") as f:
            f.write(txt)
    return path
