"""The parsers the binding tests share: the C headers' functions and structs, the C# bindings' imports and structs (CS, c_functions,
cs_imports, KINDS, ...), imports_of for the multi bindings, and the status names of vorbispizza_multi.h (vpzm_statuses)."""
import os
import re


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INC = os.path.join(ROOT, "include")
CS = os.path.join(ROOT, "bindings", "csharp")


def strip_c_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def strip_cs_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- kinds: what has to agree between a C parameter and its C# counterpart for the call to be ABI-correct
def c_kind(decl):
    decl = decl.strip()
    if "*" in decl:
        return "ptr"
    base = re.sub(r"\bconst\b", "", decl).split()
    base = [t for t in base if t]
    ty = base[0] if len(base) == 1 else " ".join(base[:-1])  # drop the parameter name
    return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "float": "f32", "void": "void",
            "uint8_t": "u8", "uint16_t": "u16", "int16_t": "i16", "double": "f64"}[ty]


def cs_kind(decl):
    decl = decl.strip()
    toks = decl.split()
    if toks[0] in ("out", "ref"):
        return "ptr"
    ty = toks[0]
    if ty.endswith("*") or (len(toks) > 1 and toks[1].startswith("*")):
        return "ptr"
    if ty in ("IntPtr", "ContextHandle", "DecoderHandle"):
        return "ptr"
    return {"int": "i32", "long": "i64", "ulong": "u64", "float": "f32", "void": "void", "byte": "u8", "short": "i16",
            "ushort": "u16", "double": "f64"}[ty]


def c_functions(header, prefix):
    text = strip_c_comments(open(os.path.join(INC, header)).read())
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w \t\*]*?)\b(%s\w+)\s*\(([^;{]*?)\)\s*;" % prefix, text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = [] if args in ("void", "") else [a.strip() for a in args.split(",")]
        out[name] = (c_kind(ret.strip() + " x") if "*" not in ret else "ptr", [c_kind(p) for p in params])
    return out


def cs_imports(path):
    text = strip_cs_comments(open(path).read())
    out = {}
    pat = r"\[DllImport\((\w+)[^\]]*\)\]\s*(?:public|private|internal)?\s*static\s+extern\s+([\w\*]+)\s+(\w+)\s*\(([^;]*?)\)\s*;"
    for m in re.finditer(pat, text, flags=re.S):
        lib, ret, name, args = m.group(1), m.group(2), m.group(3), " ".join(m.group(4).split())
        params = [] if not args else [a.strip() for a in args.split(",")]
        out[name] = (lib, cs_kind(ret + " x"), [cs_kind(p) for p in params])
    return out


# ---- structs
def c_structs(header):
    text = strip_c_comments(open(os.path.join(INC, header)).read())
    defines = {k: int(v, 0) for k, v in re.findall(r"#define\s+(\w+)\s+(\(?-?\w+\)?)\s*$", text, flags=re.M)
               if re.fullmatch(r"\(?-?(0x[0-9a-fA-F]+|\d+)\)?", v) for v in [v.strip("()")]}
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            # "int32_t a, b" / "const T *p" / "uint8_t x[EXPR]"
            mm = re.match(r"^(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", stmt)
            ty, star, names = mm.group(1), mm.group(2), mm.group(3)
            for n in [x.strip() for x in names.split(",")]:
                arr = re.match(r"(\w+)\[(.+)\]", n)
                if arr:
                    expr = arr.group(2)
                    for k, v in defines.items():
                        expr = re.sub(r"\b%s\b" % k, str(v), expr)
                    fields.append((arr.group(1), c_kind(ty + " x"), int(eval(expr))))
                else:
                    ptr = bool(star) or n.startswith("*")
                    fields.append((n.lstrip("*").strip(), "ptr" if ptr else c_kind(ty + " x"), 0))
        out[m.group(1)] = fields
    return out, defines


def cs_structs(path):
    text = strip_cs_comments(open(path).read())
    out = {}
    for m in re.finditer(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*public\s+struct\s+(\w+)\s*\{(.*?)\}", text, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            stmt = re.sub(r"^public\s+", "", stmt)
            fixed = stmt.startswith("fixed ")
            stmt = re.sub(r"^fixed\s+", "", stmt)
            ty, names = stmt.split(" ", 1)
            for n in [x.strip() for x in names.split(",")]:
                arr = re.match(r"(\w+)\[(\d+)\]", n)
                kind = "u8" if ty == "PacketFlags" else cs_kind(ty + " x")
                if arr:
                    assert fixed
                    fields.append((arr.group(1), kind, int(arr.group(2))))
                else:
                    fields.append((n, kind, 0))
        out[m.group(1)] = fields
    return out


def norm(name):
    return name.replace("_", "").lower()


def imports_of(tmp_path, name):
    """cs_imports of a binding file, the dispatcher's SafeHandle read as the pointer it marshals as"""
    text = open(os.path.join(CS, name)).read().replace("VorbisPizzaMulti.DispatcherHandle", "IntPtr")
    path = tmp_path / name
    path.write_text(text)
    return cs_imports(str(path))


def vpzm_statuses():
    """{name: value} of every VPZM_E_* of every header"""
    out = {}
    for header in sorted(os.listdir(INC)):
        text = strip_c_comments(open(os.path.join(INC, header)).read())
        for name, value in re.findall(r"#define\s+(VPZM_E_\w+)\s+\(?(-?\d+)\)?", text):
            assert out.setdefault(name, int(value)) == int(value), name
    return out
