"""ctypes binding of libctta_hip.so (the C ABI declared in include/ctta.h).

PyTorch is used above this boundary only as the owner of device memory and streams: every
call passes raw `data_ptr()`s plus the current HIP stream.  There is NO fallback: if the
library is missing or a call fails, a RuntimeError is raised (the reference raises Python
exceptions at the same places -- shape asserts, load_state_dict key errors).
"""
import ctypes
from ctypes import byref  # noqa: F401  (re-exported for callers of out-parameter entry points)
import os
import subprocess
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int16, c_int32,  # noqa: F401  (the ctypes names
                    c_int64, c_size_t, c_uint8, c_void_p)                # this module has always exported: callers build host arrays with them)

from . import _cheader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libctta_hip.so")
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "ctta.h")

# The binding is DERIVED from the header, the single declaration of the ABI (_cheader states the one rule from C type to
# ctypes): nothing here repeats a field or an argument list.  STRUCTS: C struct name -> ctypes.Structure, FUNCTIONS:
# symbol -> _cheader.Function, SIGNATURES: symbol -> (restype, argtypes), CONSTANTS: the #defines and enumerators.
with open(HEADER) as _f:
    CONSTANTS, STRUCTS, FUNCTIONS = _cheader.parse(_f.read())
SIGNATURES = {name: (f.restype, f.argtypes) for name, f in FUNCTIONS.items()}
MAX_LEVELS = CONSTANTS["CTTA_MAX_LEVELS"]
MAX_UPS = CONSTANTS["CTTA_MAX_UPS"]
Tensor = STRUCTS["ctta_tensor"]
UNetConfig = STRUCTS["ctta_unet_config"]
VAEConfig = STRUCTS["ctta_vae_config"]
T5Config = STRUCTS["ctta_t5_config"]
HifiganConfig = STRUCTS["ctta_hifigan_config"]
FfnDesc = STRUCTS["ctta_ffn_desc"]
ConvDesc = STRUCTS["ctta_conv_desc"]
ConvPlanEnv = STRUCTS["ctta_conv_plan_env"]
ConvPlanInfo = STRUCTS["ctta_conv_plan_info"]
WgradGeom = STRUCTS["ctta_wgrad_geom"]
WgradPolicy = STRUCTS["ctta_wgrad_policy"]
WgradPlanInfo = STRUCTS["ctta_wgrad_plan_info"]
LoraFwdSite = STRUCTS["ctta_lora_fwd_site"]
LoraBwdSite = STRUCTS["ctta_lora_bwd_site"]
ResampleClip = STRUCTS["ctta_resample_clip"]
PackJob = STRUCTS["ctta_pack_job"]
CopySeg = STRUCTS["ctta_copy_seg"]
TposeJob = STRUCTS["ctta_tpose_job"]

_lib = None


def build(force=False):
    """Compiles csrc/*.hip for gfx950 into consistencytta_amd/libctta_hip.so (in-tree)."""
    if force:
        for f in os.listdir(os.path.join(CSRC, "build")) if os.path.isdir(os.path.join(CSRC, "build")) else []:
            os.remove(os.path.join(CSRC, "build", f))
    subprocess.run(["bash", os.path.join(CSRC, "build.sh")], check=True)
    return LIB_PATH


def lib():
    """Loads the library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libctta_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or consistencytta_amd/csrc/build.sh; there is no non-HIP fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64; import torch first so that this library binds to the SAME HIP runtime
    # instance (loading ours first pulls in /opt/rocm's copy: two runtimes in one process, device memory of one is
    # invisible to the other -- observed as "no ROCm-capable device is detected" from the second one)
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    # CTTA_OPT_<NAME>=<int> in the environment of the PYTHON process sets a library option at load time (A/B scripts:
    # tools/gpu_call.sh ab).  The library itself reads no environment variable; see ctta_set_option in include/ctta.h.
    for i in range(L.ctta_num_options()):
        name = L.ctta_option_name(i).decode()
        v = os.environ.get("CTTA_OPT_" + name.upper())
        if v is not None:
            set_option(name, int(v))
    return L


def set_option(name, value):
    """ctta_set_option (include/ctta.h): the library's only switches."""
    check(lib().ctta_set_option(name.encode(), int(value)))


def get_option(name):
    v = c_int()
    check(lib().ctta_get_option(name.encode(), ctypes.byref(v)))
    return v.value


def options():
    L = lib()
    return {L.ctta_option_name(i).decode(): get_option(L.ctta_option_name(i).decode()) for i in range(L.ctta_num_options())}


class CttaError(RuntimeError):
    pass


def check(status):
    if status != 0:
        msg = lib().ctta_last_error()
        raise CttaError("ctta status %d: %s" % (status, msg.decode() if msg else "?"))


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def tensor_table(sd):
    """dict name -> contiguous fp32 CUDA tensor  =>  (ctypes array of ctta_tensor, keepalive)."""
    import torch
    n = len(sd)
    arr = (Tensor * n)()
    keep = []
    for i, (k, v) in enumerate(sd.items()):
        if v.dtype != torch.float32 or not v.is_cuda:
            raise CttaError("weight '%s' must be a float32 CUDA tensor (got %s on %s)" % (k, v.dtype, v.device))
        v = v.contiguous()
        kb = k.encode()
        keep.append((kb, v))
        arr[i].name = kb
        arr[i].data = v.data_ptr()
        arr[i].ndim = v.ndim
        for d in range(v.ndim):
            arr[i].shape[d] = v.shape[d]
    return arr, keep


def param_table(named):
    """(name, parameter) pairs  =>  `tensor_table` of the detached parameters; each must already live on the device."""
    sd = {}
    for k, p in named:
        if not p.is_cuda:
            raise CttaError("parameter '%s' is on %s: the HIP engine has no CPU path" % (k, p.device))
        sd[k] = p.detach()
    return tensor_table(sd)


class EngineHandle:
    """Owner of one native engine handle (ctta_unet / vae / vae_encoder / hifigan / t5): the handle, the capacity tuple it
    was created for, the identity key (extent, flags, device) and the weights version it packed.  WHEN a handle is replaced
    is the caller's policy, expressed in what it passes to `fits` / `replace`; a captured hipGraph holds the handle's
    address, so a replacement invalidates every graph recorded through it."""

    def __init__(self, destroy):
        self.destroy = destroy          # name of the ctta_*_destroy symbol
        self.h = self.capacity = self.key = self.version = None

    def fits(self, capacity, key, version):
        """A live handle of this identity and weights version whose every capacity covers the request."""
        return (self.h is not None and key == self.key and version == self.version
                and all(n <= c for n, c in zip(capacity, self.capacity)))

    def replace(self, create_fn, capacity, key, version, device):
        """Destroys the old handle FIRST (two generations never hold device memory together), then
        `create_fn(out_handle) -> status` on `device`.  A failed create leaves the holder empty."""
        import torch
        self.release()
        h = c_void_p()
        with torch.cuda.device(device):
            check(create_fn(h))
        self.h, self.capacity, self.key, self.version = h, tuple(capacity), key, version
        return h

    def release(self):
        h, self.h = self.h, None
        if h:
            getattr(lib(), self.destroy)(h)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def read_taps(prefix, handle, device):
    """name -> NCHW fp32 tensor of every intermediate a debug_taps handle recorded (`prefix`: "ctta_unet", ...)."""
    import torch
    from collections import OrderedDict
    L = lib()
    num, info, read = (getattr(L, "%s_%s" % (prefix, f)) for f in ("num_taps", "tap_info", "tap_read"))
    out = OrderedDict()
    for i in range(num(handle)):
        name = c_char_p()
        dims = (c_int * 4)()
        check(info(handle, i, name, dims))
        t = torch.empty(tuple(dims), dtype=torch.float32, device=device)
        check(read(handle, i, ptr(t), stream_ptr()))
        out[name.value.decode()] = t
    return out
