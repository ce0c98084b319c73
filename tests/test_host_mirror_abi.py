"""The host mirror against include/srslte_hip/phy_hip.h, as two texts of the repository: every ctypes.Structure of the package has the layout
of the typedef it names, and every row of the binding table has its prototype's parameter count, parameter classes and return class. No
library is loaded and no device is needed; the layout check compiles a few lines with gcc."""
import ctypes as C
import importlib
import os
import re

from _libs import ROOT, struct_layout

pkg = importlib.import_module("srslte-emane_amd")
INC = os.path.join(ROOT, "include")


def _header(name):
    """The header without comments and preprocessor lines."""
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, "srslte_hip", name)).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", src, flags=re.M)


PHY, COMPAT = _header("phy_hip.h"), _header("srslte_compat.h")
PROTOTYPES = {n: (" ".join(r.split()), [" ".join(a.split()) for a in args.split(",")])
              for r, n, args in re.findall(r"([\w\s\*]+?)\b(srslte_hip_\w+)\s*\(([^()]*)\)\s*;", PHY)}
TYPEDEFS = re.findall(r"\}\s*(srslte_hip_\w+_t)\s*;", PHY)


def _mirrors():
    out, todo = [], [C.Structure]
    while todo:
        for cls in todo.pop().__subclasses__():
            todo.append(cls)
            if cls.__module__.split(".")[0] == pkg.__name__:
                out.append(cls)
    return out


def test_struct_mirrors_have_the_headers_layout():
    mirrors = _mirrors()
    unnamed = [m.__name__ for m in mirrors if "C_TYPE" not in vars(m)]
    assert not unnamed, "ctypes.Structure without the C_TYPE it mirrors: %s" % unnamed
    bad = []
    for header, group in (("srslte_hip/phy_hip.h", [m for m in mirrors if m.C_TYPE in TYPEDEFS]),
                          ("srslte_hip/srslte_compat.h", [m for m in mirrors if m.C_TYPE not in TYPEDEFS])):
        if not group:
            continue
        want = struct_layout({m.C_TYPE: [f for f, *_ in m._fields_] for m in group}, [header], [INC])  # a field the header lacks fails here
        for m in group:
            body = re.search(r"\{([^{}]*)\}\s*%s\s*;" % m.C_TYPE, PHY if m.C_TYPE in TYPEDEFS else COMPAT).group(1)
            names = [re.findall(r"\w+", d)[-1] for decl in body.split(";") if decl.strip() for d in re.sub(r"\[[^\]]*\]", "", decl).split(",")]
            if names != [f for f, *_ in m._fields_]:
                bad.append("%s (%s): fields %s, the header has %s" % (m.__name__, m.C_TYPE, [f for f, *_ in m._fields_], names))
            if C.sizeof(m) != want[m.C_TYPE]:
                bad.append("%s (%s): sizeof %d, the header's is %d" % (m.__name__, m.C_TYPE, C.sizeof(m), want[m.C_TYPE]))
            for f, *_ in m._fields_:
                if getattr(m, f).offset != want["%s.%s" % (m.C_TYPE, f)]:
                    bad.append("%s.%s (%s): offset %d, the header's is %d" % (m.__name__, f, m.C_TYPE, getattr(m, f).offset, want["%s.%s" % (m.C_TYPE, f)]))
    assert not bad, "\n".join(bad)
    print("%d mirrors checked; typedefs of phy_hip.h without one: %s" % (len(mirrors), sorted(set(TYPEDEFS) - {m.C_TYPE for m in mirrors})))
    assert len(mirrors) >= 60


_WIDE = ("uint64_t", "int64_t", "size_t", "unsigned long long")


def _c_class(decl, is_param):
    """'ptr', 'float', 'double', 'i8', 'i16', 'i64', 'i32' or 'void' of a parameter declaration (with its name) or of a return type."""
    if "*" in decl or "[" in decl:
        return "ptr"
    t = re.sub(r"\bconst\b", "", decl).strip()
    t = re.sub(r"\s*\b\w+$", "", t) if is_param and " " in t else t
    if t in ("float", "double", "void"):
        return t
    return "i8" if t in ("uint8_t", "int8_t", "char") else "i16" if t in ("uint16_t", "int16_t", "short") else "i64" if t in _WIDE else "i32"


def _ctypes_class(t):
    if t is pkg.void:
        return "void"
    if t is None:
        return "i32"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "ptr"
    if t in (C.c_float, C.c_double):
        return "float" if t is C.c_float else "double"
    return {1: "i8", 2: "i16", 8: "i64"}.get(C.sizeof(t), "i32")


def test_binding_table_matches_the_prototypes():
    rows = pkg.signatures()
    assert len(PROTOTYPES) > 200
    bad = ["%s: a prototype of phy_hip.h without a row" % n for n in PROTOTYPES if n not in rows]
    for name, (res, args) in rows.items():
        if name not in PROTOTYPES:
            if not re.search(r"\b%s\s*\(" % name, COMPAT):
                bad.append("%s: a row for a function that neither header declares" % name)
            continue
        ret, params = PROTOTYPES[name]
        want = [_c_class(p, True) for p in params if p not in ("", "void")]
        got = [_ctypes_class(t) for t in args]
        if len(got) != len(want):
            bad.append("%s: %d argtypes, the prototype has %d parameters" % (name, len(got), len(want)))
        elif got != want:
            bad.append("%s: argtypes of classes %s, the prototype's are %s" % (name, got, want))
        if _ctypes_class(res) != _c_class(ret, False):
            bad.append("%s: restype of class %s, the prototype returns %s (%s)" % (name, _ctypes_class(res), _c_class(ret, False), ret))
    assert not bad, "\n".join(bad)
    print("%d rows checked against %d prototypes" % (len(rows), len(PROTOTYPES)))
