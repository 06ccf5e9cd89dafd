"""The ctypes binding is derived from include/ctta.h by consistencytta_amd/_cheader.py; here the C compiler says whether the
reader read the header as C does.  A parser must not be its own oracle, so gcc is:
  functions   one _Static_assert per declared function that the type of &NAME is RET(*)(P1, P2, ...), spelled from the reader's
              result: parameter count, order and types, `const` on pointees included;
  structs     sizeof of every struct, offsetof and size of every field, and sizeof of every scalar C type of the reader's
              map (the only hand-written type knowledge left), printed by a C program and compared with ctypes.
The rest: the reader refuses what it does not understand, and the one pointer rule takes every argument form the
repository passes."""
import ctypes
import re
import subprocess
from ctypes import POINTER, byref, c_char_p, c_int, c_void_p

import pytest

import abi
from consistencytta_amd import _cheader as H
from consistencytta_amd import _native as N

CONSTANTS, STRUCTS, FUNCTIONS = H.parse(abi.HEADER)
PUBLIC = dict(Tensor="ctta_tensor", UNetConfig="ctta_unet_config", VAEConfig="ctta_vae_config", T5Config="ctta_t5_config",
              HifiganConfig="ctta_hifigan_config", FfnDesc="ctta_ffn_desc", ConvDesc="ctta_conv_desc",
              ConvPlanEnv="ctta_conv_plan_env", ConvPlanInfo="ctta_conv_plan_info", WgradGeom="ctta_wgrad_geom",
              WgradPolicy="ctta_wgrad_policy", WgradPlanInfo="ctta_wgrad_plan_info", LoraFwdSite="ctta_lora_fwd_site",
              LoraBwdSite="ctta_lora_bwd_site", ResampleClip="ctta_resample_clip", PackJob="ctta_pack_job",
              CopySeg="ctta_copy_seg", TposeJob="ctta_tpose_job")
C_SCALARS = dict(H.SCALARS, **{"void*": c_void_p, "const char*": c_char_p, "ctta_status": c_int})


def compile_function_asserts(functions, include, tmp_path):
    """(gcc's exit status, its messages) for one assert per function against the ctta.h under `include`."""
    src = tmp_path / "functions.c"
    src.write_text('#include "ctta.h"\n' + "".join(
        '_Static_assert(__builtin_types_compatible_p(__typeof__(&%s), %s(*)(%s)), "%s");\n'
        % (name, f.c_restype, ", ".join(f.c_argtypes) or "void", name) for name, f in functions.items()))
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", include, str(src)], capture_output=True, text=True)
    return r.returncode, r.stderr


def layout_differences(structs, include, tmp_path):
    """{name: (ctypes, gcc)} wherever the two disagree: "sizeof T" of every struct and scalar, "S.f" -> (offset, size)."""
    want = {"sizeof " + t: ctypes.sizeof(c) for t, c in list(structs.items()) + list(C_SCALARS.items())}
    lines = ['  printf("%s|%%zu\\n", sizeof(%s));' % (k, k[len("sizeof "):]) for k in want]
    for s, cls in structs.items():
        for f, _ in cls._fields_:
            want["%s.%s" % (s, f)] = (getattr(cls, f).offset, getattr(cls, f).size)
            lines.append('  printf("%s.%s|%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ctta.h"\nint main(void) {\n%s\n  return 0;\n}\n' % "\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", include, str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        v = [int(x) for x in line.split("|")[1].split()]
        got[line.split("|")[0]] = v[0] if len(v) == 1 else tuple(v)
    assert sorted(want) == sorted(got)
    return {k: (want[k], got[k]) for k in want if want[k] != got[k]}


def test_reader_reads_the_whole_header():
    assert sorted(FUNCTIONS) == abi.declared_symbols() and len(FUNCTIONS) >= 218
    assert list(STRUCTS) == re.findall(r"\}\s*(ctta_\w+)\s*;", re.sub(r"enum\s*\{[^}]*\}\s*\w*\s*;", "", abi.CODE))
    assert len(STRUCTS) >= 18 and set(PUBLIC.values()) == set(STRUCTS)
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(CTTA_\w+)\s+(\d+)", abi.CODE)}
    assert defines and all(CONSTANTS[k] == v for k, v in defines.items())
    assert (CONSTANTS["CTTA_MAX_LEVELS"], CONSTANTS["CTTA_MAX_UPS"], CONSTANTS["CTTA_PAIR_MAX"]) == (4, 8, 256)
    assert (CONSTANTS["CTTA_OK"], CONSTANTS["CTTA_ERR_NOMEM"], CONSTANTS["CTTA_WGRAD_IM2COL_T"]) == (0, 4, 5)


def test_functions_are_what_the_compiler_reads(tmp_path):
    rc, err = compile_function_asserts(FUNCTIONS, abi.INCLUDE, tmp_path)
    assert rc == 0, err


def test_structs_and_scalars_are_what_the_compiler_lays_out(tmp_path):
    diff = layout_differences(STRUCTS, abi.INCLUDE, tmp_path)
    assert not diff, "name: (ctypes, compiler) %r" % diff
    fields = lambda s: dict(STRUCTS[s]._fields_)                          # noqa: E731
    assert fields("ctta_tensor") == dict(name=c_char_p, data=c_void_p, ndim=c_int, shape=ctypes.c_int64 * 4)
    assert fields("ctta_hifigan_config")["resblock_dilations"] is (c_int * 3) * 4         # int resblock_dilations[4][3]
    assert fields("ctta_pack_job")["col_aux"] is c_void_p and fields("ctta_unet_config")["heads"] is c_int * N.MAX_LEVELS


def test_native_binds_the_readers_result():
    lib = abi.built_lib()
    assert sorted(N.SIGNATURES) == abi.declared_symbols()
    for name, f in FUNCTIONS.items():
        mine = N.FUNCTIONS[name]             # N's own parse: same spelling as this module's, hence (one rule) the same types
        assert (mine.c_restype, mine.c_argtypes) == (f.c_restype, f.c_argtypes), name
        assert N.SIGNATURES[name] == (mine.restype, mine.argtypes), name
        fn = getattr(lib, name)              # AttributeError: declared but not exported
        assert fn.restype is mine.restype and list(fn.argtypes) == mine.argtypes, name
    assert all(getattr(N, py) is N.STRUCTS[c] for py, c in PUBLIC.items())
    assert (N.MAX_LEVELS, N.MAX_UPS) == (4, 8)
    assert lib.ctta_version() == 100 and lib.ctta_conv_gemm_num_variants() >= 4


def test_one_rule_for_every_function():
    """The same C spelling is the same ctypes class wherever it occurs, and the classes are the documented ones."""
    seen = {}
    for name, f in N.FUNCTIONS.items():
        for spelling, t in zip([f.c_restype] + f.c_argtypes, [f.restype] + f.argtypes):
            assert seen.setdefault(spelling, t) is t, (name, spelling)
    ptr = lambda s: H.struct_pointer(N.STRUCTS[s])                      # noqa: E731
    want = {"void": None, "int": c_int, "ctta_status": c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double, "const char*": c_char_p, "const char**": POINTER(c_char_p),
            "int[4]": POINTER(c_int * 4), "void*": c_void_p, "const void*": c_void_p, "const float*": c_void_p, "int*": c_void_p,
            "double*": c_void_p, "size_t*": c_void_p, "const int32_t*": c_void_p, "ctta_unet*": c_void_p,
            "const ctta_unet*": c_void_p, "ctta_unet**": POINTER(c_void_p), "void**": POINTER(c_void_p),
            "const void* const*": POINTER(c_void_p), "const ctta_tensor*": ptr("ctta_tensor"),
            "const ctta_conv_desc*": ptr("ctta_conv_desc"), "const ctta_ffn_desc*": ptr("ctta_ffn_desc"),
            "ctta_ffn_desc*": ptr("ctta_ffn_desc"), "const ctta_pack_job*": ptr("ctta_pack_job")}
    assert {k: seen[k] for k in want} == want


# header text the reader must refuse -> the part of it that the message must quote
REFUSED = {
    "int ctta_f(uint16_t x);": "ctta_f(uint16_t x)",                                          # unknown type name
    "typedef struct { long n; } ctta_s;": "long n",
    "typedef struct { int a; } ctta_a;\ntypedef struct { ctta_a inner; int b; } ctta_b;": "ctta_a inner",   # struct by value
    "typedef struct { int a; } ctta_a;\nint ctta_f(ctta_a a);": "ctta_f(ctta_a a)",
    "typedef struct { int a; } ctta_a;\ntypedef struct { const ctta_a* p; } ctta_b;": "const ctta_a* p",
    "typedef union { int a; float b; } ctta_u;": "typedef union",
    "typedef struct { union { int a; float b; } u; } ctta_s;": "union { int a",
    "typedef struct { int a : 3; int b; } ctta_s;": "int a : 3",                              # bit-field
    "int ctta_f(void (*cb)(int), void* user);": "(*cb)(int)",                                 # function pointers
    "typedef struct { int (*cb)(void); } ctta_s;": "int (*cb)(void)",
    "int ctta_f(const char* fmt, ...);": "fmt, ...",                                          # variadic list
    "typedef struct { int a[CTTA_N]; } ctta_s;": "int a[CTTA_N]",
    "#define CTTA_X 1.5": "CTTA_X 1.5",
    "int ctta_f(void)": "int ctta_f(void)",                                                   # text left over
}


@pytest.mark.parametrize("text", sorted(REFUSED), ids=lambda t: re.sub(r"\W+", "_", REFUSED[t]).strip("_"))
def test_reader_raises_on_what_it_does_not_read(text):
    with pytest.raises(H.HeaderError) as e:
        H.parse("#include <stdint.h>\n/* a comment */\nint ctta_ok(int a, const float* p);\n" + text + "\n")
    assert REFUSED[text] in str(e.value), str(e.value)


def test_pointer_rule_takes_every_argument_form_in_use():
    """Through the from_param of the derived argtypes, as a call would; the last part calls a pure host function."""
    arg = lambda name, i: N.SIGNATURES[name][1][i]                      # noqa: E731
    # a pointer to a header struct: an instance, byref, an array (host tables) and a raw address (device tables)
    desc, d = arg("ctta_conv_plan", 0), N.ConvDesc()
    for ok in (None, 0, 1 << 40, c_void_p(4096), byref(d), d, (N.ConvDesc * 3)(), ctypes.pointer(d)):
        desc.from_param(ok)
    for bad in (N.ConvPlanEnv(), byref(N.ConvPlanEnv()), (N.Tensor * 2)(), 1.5, b"bytes"):
        with pytest.raises((TypeError, ctypes.ArgumentError)):
            desc.from_param(bad)
    arg("ctta_unet_create", 1).from_param((N.Tensor * 4)())
    arg("ctta_unet_create", 0).from_param(N.UNetConfig())
    for name, i in (("ctta_pack_weight_multi", 0), ("ctta_copy_segments_multi", 0), ("ctta_transpose_multi", 0), ("ctta_resample_sinc", 2)):
        arg(name, i).from_param(c_void_p(1 << 40))                      # N.ptr(device table)
    # pointers to scalars, to void and to opaque handles are c_void_p: byref, arrays, addresses; not a bare c_int()
    for name, i in (("ctta_get_option", 1), ("ctta_prof_collect", 1), ("ctta_prof_collect", 3), ("ctta_conv_bound_workspace", 1),
                    ("ctta_unet_backward_next", 4), ("ctta_lora_sites_supported", 1), ("ctta_lsd", 5), ("ctta_unet_destroy", 0)):
        assert arg(name, i) is c_void_p, name
    for ok in (None, 4096, c_void_p(4096), byref(c_int()), byref(ctypes.c_double()), byref(ctypes.c_int64()),
               byref(ctypes.c_size_t()), (c_int * 3)(1, 2, 3), (ctypes.c_int32 * 2)()):
        c_void_p.from_param(ok)
    with pytest.raises(TypeError):
        c_void_p.from_param(c_int())
    # const char*: bytes or None; T**: a bare c_void_p(), byref or an array; const char** and int dims[4] as read_taps passes them
    assert arg("ctta_prof_collect", 4) is c_char_p and arg("ctta_set_option", 0) is c_char_p
    c_char_p.from_param(b"launches.csv"), c_char_p.from_param(None)
    out = arg("ctta_unet_create", 4)
    assert out is arg("ctta_conv_bound_workspace", 0) is arg("ctta_reschain_conv1d", 6)
    for ok in (c_void_p(), byref(c_void_p()), (c_void_p * 3)()):
        out.from_param(ok)
    arg("ctta_unet_tap_info", 2).from_param(c_char_p())
    arg("ctta_unet_tap_info", 3).from_param((c_int * 4)())
    with pytest.raises(TypeError):
        arg("ctta_unet_tap_info", 3).from_param((c_int * 3)())
    # the raw address arrives: ctta_conv_plan is a pure host function, so a host struct's address can stand in for a device one
    d.x0 = d.w = d.out = 0x1000
    d.c0, d.batch, d.n, d.ldc, d.k_pad, d.alpha = 320, 4096, 320, 320, 320, 1.0
    d.hi = d.wi = d.ho = d.wo = d.kh = d.kw = d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1
    env = N.ConvPlanEnv(cu_count=256, xcd=1, splitk=1, streamk=1, workspace_bytes=192 << 20, workspace_header_zeroed=1)
    plans = []
    for form in (byref(d), d, ctypes.addressof(d), c_void_p(ctypes.addressof(d))):
        info = N.ConvPlanInfo()
        assert abi.built_lib().ctta_conv_plan(form, env, byref(info)) == 0
        plans.append(bytes(info))
    assert len(set(plans)) == 1 and any(plans[0])
