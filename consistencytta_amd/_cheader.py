"""Reader of include/ctta.h: the C header is the single declaration of the ABI, and the ctypes binding is derived from it.

`parse(text)` returns (constants, structs, functions):
  constants  name -> int: every `#define NAME <integer>` and every enumerator
  structs    C name -> ctypes.Structure subclass, in header order
  functions  name -> Function(restype, argtypes, c_restype, c_argtypes); the c_* members are the normalised C spelling of the
             return type and of every parameter type ("const ctta_tensor*", "int[4]"), which a C compiler can be asked to
             compare with its own reading of the header (tests/test_abi_cpu.py).

This is not a C parser.  It reads the subset the header is written in -- comments, include guards, integer #defines, enums,
`typedef struct NAME NAME;` handles, `typedef struct [NAME] { scalars, arrays, pointers } NAME;` and prototypes -- and raises
HeaderError, quoting the declaration, for everything else: an unknown type name, a struct or union by value, a bit-field, a
function pointer, a variadic list.  It never guesses.

ONE rule maps a C type to ctypes, in every function and every struct:
  scalar                      by name (SCALARS); an enum type is c_int
  T x[N][M] (struct field)    ((c_T * M) * N)
  T x[N] (parameter)          POINTER(c_T * N)
  const char*                 c_char_p;  const char** (parameter): POINTER(c_char_p)
  any other T** (parameter)   POINTER(c_void_p): out-handles, host tables of device pointers
  S* (parameter), S a struct  struct_pointer(S): what POINTER(S) takes (an instance, byref, an array of S) and also a raw
                              address (int, c_void_p), because job tables live in device memory
  any other T*                c_void_p: void, scalars, opaque handles.  It takes byref(...), arrays, addresses and None, and
                              refuses a bare c_int(): out-parameters are passed with byref
A struct field may point to void, to a scalar or to const char, and to nothing else.
"""
import ctypes
import re
from collections import namedtuple
from ctypes import POINTER, c_char_p, c_int, c_void_p

SCALARS = {"int": c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64,
           "int32_t": ctypes.c_int32, "int16_t": ctypes.c_int16, "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t}
Function = namedtuple("Function", "restype argtypes c_restype c_argtypes")
_DECLARATOR = r"((?:\*\s*(?:const\s*)?)*)(\w+)?\s*((?:\[\s*\w+\s*\]\s*)*)"      # `* const * name [N][M]`
_DECLARATION, _DECLARATOR = re.compile(r"(const\s+)?(\w+)\s*" + _DECLARATOR), re.compile(_DECLARATOR)
_struct_pointers = {}


class HeaderError(ValueError):
    pass


def struct_pointer(S):
    """The parameter type of `S*`: POINTER(S) that also takes a raw address."""
    if S not in _struct_pointers:
        typed, raw = POINTER(S).from_param, c_void_p.from_param

        class StructPointer(POINTER(S)):
            @classmethod
            def from_param(cls, obj):       # Python-level: about 0.2 us per argument more than POINTER(S)'s own
                return raw(obj) if isinstance(obj, (int, c_void_p)) else typed(obj)

        _struct_pointers[S] = StructPointer
    return _struct_pointers[S]


class _Reader:
    def __init__(self):
        self.constants, self.structs, self.functions, self.enums, self.handles = {}, {}, {}, set(), set()

    def number(self, tok, where):
        if not tok.isdigit() and tok not in self.constants:
            raise HeaderError("'%s' is not an integer constant in: %s" % (tok, where))
        return int(tok) if tok.isdigit() else self.constants[tok]

    def declare(self, text, where, param, base=None):
        """One declaration (`base`: a further declarator of a comma list) -> (name, ctypes type, C spelling, base)."""
        m = (_DECLARATION if base is None else _DECLARATOR).fullmatch(text.strip())
        if not m:
            raise HeaderError("cannot read '%s' (function pointer, bit-field, variadic list, ...) in: %s" % (text.strip(), where))
        const, typ = base or (bool(m.group(1)), m.group(2))
        stars, name, dims = m.groups()[-3:]
        ptrs = re.findall(r"\*\s*(const)?", stars)
        dims = [self.number(n, where) for n in re.findall(r"\w+", dims)]
        known = typ in SCALARS or typ in ("void", "char") or typ in self.enums or typ in self.handles or typ in self.structs
        if not known:
            raise HeaderError("unknown type '%s' in: %s" % (typ, where))
        spelling = ("const " if const else "") + typ + "".join("* const" if c else "*" for c in ptrs) + "".join("[%d]" % n for n in dims)
        return name, self.ctype(const, typ, len(ptrs), dims, param, where), spelling, (const, typ)

    def ctype(self, const, typ, depth, dims, param, where):
        """The rule of the module docstring."""
        if typ == "char":
            if const and not dims and (depth == 1 or (depth == 2 and param)):
                return c_char_p if depth == 1 else POINTER(c_char_p)
        elif depth == 0 and (typ in SCALARS or typ in self.enums) and len(dims) <= (1 if param else 2):
            t = SCALARS.get(typ, c_int)
            for n in reversed(dims):
                t = t * n
            return POINTER(t) if param and dims else t
        elif depth == 1 and not dims and (param or typ == "void" or typ in SCALARS):
            return struct_pointer(self.structs[typ]) if typ in self.structs else c_void_p
        elif depth == 2 and not dims and param:
            return POINTER(c_void_p)
        raise HeaderError("no rule for this type (by value, as a field or at this depth) in: %s" % where)

    def struct(self, name, body, where):
        fields = []
        for member in filter(str.strip, body.split(";")):
            first, base = True, None
            for part in member.split(","):              # comma list: `int a, b[4];`, `const int32_t *p, *q;`
                fname, t, _, base = self.declare(part, "%s in %s" % (" ".join(member.split()), where), False, None if first else base)
                first = False
                if fname is None:
                    raise HeaderError("member without a name: %s in %s" % (" ".join(member.split()), where))
                fields.append((fname, t))
        self.structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "%s (include/ctta.h)" % name})

    def function(self, stmt):
        m = re.fullmatch(r"([^()]*?)\b(\w+)\s*\(([^()]*)\)", stmt)
        if not m or m.group(2) in self.functions:
            raise HeaderError("not a declaration this reader knows: %s" % stmt)
        rname, restype, c_restype, _ = (None, None, "void", None) if m.group(1).strip() == "void" else self.declare(m.group(1), stmt, True)
        if rname is not None or "[" in c_restype:
            raise HeaderError("bad return type in: %s" % stmt)
        params = [] if m.group(3).strip() == "void" else [self.declare(p, stmt, True) for p in m.group(3).split(",")]
        self.functions[m.group(2)] = Function(restype, [p[1] for p in params], c_restype, [p[2] for p in params])

    def statement(self, stmt):
        stmt = " ".join(stmt.split())
        handle = re.fullmatch(r"typedef struct (\w+) (\w+)", stmt)
        struct = re.fullmatch(r"typedef struct ?(\w*) ?\{([^{}]*)\} ?(\w+)", stmt)
        enum = re.fullmatch(r"(typedef )?enum ?\{([\w\s=,]*)\} ?(\w*)", stmt)
        if handle and handle.group(1) == handle.group(2):
            self.handles.add(handle.group(1))
        elif struct and struct.group(1) in ("", struct.group(3)):
            self.struct(struct.group(3), struct.group(2), "typedef struct { ... } " + struct.group(3))
        elif enum and bool(enum.group(1)) == bool(enum.group(3)):
            value = -1
            for name, v in re.findall(r"(\w+) ?(?:= ?(\w+))?", enum.group(2)):
                value = self.constants[name] = self.number(v, stmt) if v else value + 1
            self.enums.update(filter(None, [enum.group(3)]))
        elif re.match(r"(typedef|struct|union|enum)\b", stmt) or "{" in stmt:
            raise HeaderError("not a declaration this reader knows: %s" % stmt)
        else:
            self.function(stmt)

    def preprocessor(self, line):
        m = re.fullmatch(r"#\s*define\s+(\w+)\s+(\d+)", line)
        if m:
            self.constants[m.group(1)] = int(m.group(2))
        elif not re.fullmatch(r"#\s*(ifndef\s+\w+|ifdef\s+__cplusplus|endif|define\s+\w+|include\s*<(stddef|stdint)\.h>)", line):
            raise HeaderError("unsupported preprocessor line: %s" % line)


def parse(text):
    """Header text -> (constants, structs, functions); see the module docstring."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    rd, code, depth, extern_c = _Reader(), [], 0, 0
    for line in text.split("\n"):
        between = not depth and not "".join(code).strip()
        if between and line.strip().startswith("#"):
            rd.preprocessor(line.strip())
        elif between and re.fullmatch(r'\s*extern\s+"C"\s*\{\s*', line):         # the pair that __cplusplus guards
            extern_c += 1
        elif between and extern_c and line.strip() == "}":
            extern_c -= 1
        else:
            for piece in re.split(r"([;{}])", line + "\n"):
                if piece == ";" and depth == 0:
                    rd.statement("".join(code))
                    code = []
                else:
                    depth += (piece == "{") - (piece == "}")
                    code.append(piece)
    if depth or extern_c or "".join(code).strip():
        raise HeaderError("text left over at the end: %s" % " ".join("".join(code).split())[:200])
    return rd.constants, rd.structs, rd.functions
