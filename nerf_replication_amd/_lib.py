"""ctypes binding of libnerf_mi355x.so (include/nerf_mi355x.h and, for the small-network entries, include/nerf_mi355x_nn.h).  Plumbing only: device memory,
streams and error translation.  Fails loudly when the library is missing -- no fallback."""
import ctypes
import os
import subprocess

import torch  # noqa: F401  (imported first so that the HIP runtime torch loaded is the one we bind to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnerf_mi355x.so")
CSRC = os.path.join(_HERE, "csrc")

N_SAMPLES = 64
N_IMPORTANCE = 128
PREC_F32 = 0
PREC_F16 = 1
PREC_F32X = 2
PREC_F16S = 3          # fp16 arithmetic on 16x16x32 MFMA tiles (A/B partner of PREC_F16's 32x32x16 tiles)
# "f16" is the fp16-activation path of BASELINE config 5.  Both MFMA shapes are built and tested; the 16x16x32 kernel measured
# 0.3-0.9 % (fine launch) / 3 % (coarse launch) faster in interleaved A/Bs (profiles/r03_f16_variants.csv) and is what "f16"
# selects; "f16m32" selects the 32x32x16 kernel explicitly.
PRECISIONS = {"f32": PREC_F32, "fp32": PREC_F32, "f16": PREC_F16S, "fp16": PREC_F16S, "f16s": PREC_F16S, "f16m32": PREC_F16, "f32x": PREC_F32X}


def fp32_accurate(precision_name: str) -> bool:
    """The precisions with fp32-accurate arithmetic: what stochastic sampling, occupancy culling and the gradient chain run in."""
    return PRECISIONS[precision_name] in (PREC_F32, PREC_F32X)


# The binding surface, one line per entry of include/nerf_mi355x.h: "name  return kind : one kind per parameter".  Kinds:
#   i32 i64 f32 f64            scalars
#   f32* i32* u8* i64* f64*    device pointer to elements of that type (uint32_t* is i32*: the bitfields are int32 tensors);
#   void*                      device bytes of any element type (packed models, workspaces)
#   T[N] / T[]                 HOST array of N (any number of) scalars;  f32*[N] / f32*[]: HOST array of device float pointers
#   stream                     the trailing hipStream_t, which call() supplies
# Return kinds: status (the int32_t nerf_status of an entry that takes a stream), i32, i64, str.  tests/test_abi_symbols.py parses
# the header and compares every declaration with this table, kind by kind.
_TABLE = """
nerf_abi_version  i32 :
nerf_build_flags  i32 :
nerf_last_error  str :
nerf_packed_model_bytes  i64 : i32
nerf_pack_model  status : f32*[24] void* i32 stream
nerf_positional_encoding  status : f32* i64 i32 f32* stream
nerf_mlp_forward  status : f32* f32* i64 i32 void* f32* i32 stream
nerf_mlp_forward_rays  status : f32* f32* f32* i64 i64 i32 void* f32* i32 stream
nerf_mlp_forward_rays_for_compositing  status : f32* f32* f32* i64 i64 i32 void* f32* i32 stream
nerf_mlp_forward_rays_density  status : f32* f32* f32* i64 i64 i32 void* f32* i32 stream
nerf_composite_backward  status : f32* f32* i64 i64 i32 i32 f32* f32* f32* f32* stream
nerf_sample_fine_backward  status : f32* f32* f32* i64 f32* f32* f32* stream
nerf_adam_step  status : i32 f32*[] f32*[] f32*[] f32*[] i64[] f64 f64 f64 f64 f64 f64 i64 stream
nerf_train_grad_floats  i64 : i64
nerf_train_live_count_offset  i64 : i64
nerf_packed_bwd_bytes  i64 : i32
nerf_pack_model_bwd  status : f32*[24] void* i32 stream
nerf_mlp_backward  status : f32* f32* f32* i64 i64 i32 void* f32* f32* f32* f32* f32*[24] i32 stream
nerf_mlp_forward_rays_save_density  status : f32* f32* f32* i64 i64 i32 void* f32* f32* i32 stream
nerf_mlp_backward_density  status : f32* f32* f32* i64 i64 i32 void* f32* f32* f32* f32* f32*[24] i32 stream
nerf_mlp_forward_points_save  status : f32* f32* i64 i32 void* f32* f32* i32 stream
nerf_mlp_backward_points  status : f32* i64 i32 void* f32* f32* f32* f32* f32*[24] i32 stream
nerf_viewdirs_backward  status : f32* i64 i32 f32* f32* f32* stream
nerf_wgrad  status : f32* i64 i32 i32 f32* i64 i32 i32 f32* i64 i32 f32* i64 stream
nerf_train_save_floats  i64 : i64
nerf_mlp_forward_rays_save  status : f32* f32* f32* i64 i64 i32 void* f32* f32* i32 stream
nerf_mlp_forward_rays_save_for_compositing  status : f32* f32* f32* i64 i64 i32 void* f32* f32* i32 stream
nerf_sample_fine  status : f32* f32* f32* i64 f32* f32* u8* f32 f32 stream
nerf_composite  status : f32* f32* i64 i64 i32 i32 f32* f32* f32* stream
nerf_generate_rays  status : f64[12] i32 i32 f64 i64 i64 i64* f32* f32* stream
nerf_image_metrics  status : f32* f32* i64 f64* stream
nerf_image_ssim  status : f32* f32* i32 i32 f64* stream
nerf_render_workspace_bytes  i64 : i64 i32 i32
nerf_render_forward  status : f32* f32* i64 void* void* f32* f32* i32 i32 i32 i32 f32 void* i64 f32* f32* stream
nerf_stratified_samples  status : f32* f32* i64 f32* stream
nerf_sample_fine_rays  status : f32* f32* i64 f32* i64 i64 f32* f32* u8* f32 f32 stream
nerf_sample_fine_rays_backward  status : f32* f32* i64 f32* i64 i64 f32* f32* f32* stream
nerf_render_stochastic_workspace_bytes  i64 : i64 i32
nerf_render_forward_stochastic  status : f32* f32* i64 void* void* f32* f32* f32* f32* i32 i32 i32 i32 f32 void* i64 f32* f32* stream
nerf_mlp_backward_rays_x  status : f32* f32* f32* i64 i64 i32 void* f32* f32* f32* f32* f32* f32*[24] i32 i32 stream
nerf_rays_viewdirs_backward  status : f32* i64 i32 f32* f32* f32* stream
nerf_rays_backward  status : i64 f32* i64 f32* f32* f32* f32* f32* f32* stream
nerf_compact_valid_workspace_bytes  i64 : i64
nerf_compact_valid  status : u8* i64 i32* i32* void* stream
nerf_mlp_forward_rays_save_masked  status : f32* f32* f32* i64 i64 i32 i32* i32* void* f32* f32* i32 stream
nerf_mlp_backward_masked_workspace_bytes  i64 : i64
nerf_mlp_backward_masked  status : f32* f32* f32* i64 i64 i32 i32* i32* void* f32* f32* f32* f32* f32*[24] i32 void* stream
nerf_isosurface_workspace_bytes  i64 : i32 i32 i32
nerf_isosurface_count  status : f32* i64 i32 i32 i32 f32 void* i32* stream
nerf_isosurface_emit  status : f32* i64 i32 i32 i32 f32 f64[3] f64[3] void* f32* i32* stream
nerf_occupancy_words  i64 : i32 i32 i32
nerf_occupancy_build  status : f32* i64 i32 i32 i32 f32 i32 i32* stream
nerf_occupancy_mark  status : f32* f32* f32* i64 i64 i32 i32* i32[3] f32[3] f32[3] i32 u8* stream
nerf_occupancy_age  status : f32* i64 i64 f32 i32 u8* f32* stream
nerf_render_occupancy_workspace_bytes  i64 : i64 i32 i32
nerf_render_forward_occupancy  status : f32* f32* i64 void* void* f32* f32* i32 i32 i32 i32 f32 i32* i32* i32[3] f32[3] f32[3] i64* void* i64 f32* f32* stream
nerf_density_gradient_point_bytes  i64 :
nerf_density_gradient  status : f32* f32* f32* i64 i64 i32 void* void* i32 f32* f32* i32 void* i64 stream
nerf_composite_normals  status : f32* f32* i64 i64 i32 f32* f32* f32* stream
nerf_mesh_components_workspace_bytes  i64 : i64 i64
nerf_mesh_components  status : i32* i64 i64 void* i32* i32* i32* i32* i32* i32* stream
nerf_mesh_filter_count  status : i32* i32* u8* i64 i64 void* i32* stream
nerf_mesh_filter_emit  status : f32* i32* i64 i64 void* f32* i32* i32* stream
nerf_hashgrid_forward  status : f32* f32* i64 i32 i32 i32 i32[] f32[] f32* stream
nerf_hashgrid_backward  status : f32* f32* f32* i64 i32 i32 i32 i32[] f32[] f32* f32* stream
"""
def _parse_table(table):
    """{name: (return kind, (parameter kinds))} of a binding table, in its order."""
    signatures = {}
    for line in table.strip().splitlines():
        head, _, kinds = line.partition(":")
        signatures[head.split()[0]] = (head.split()[1], tuple(kinds.split()))
    return signatures


SIGNATURES = _parse_table(_TABLE)
EXPORTS = tuple(SIGNATURES)

_SCALAR = {"i32": ctypes.c_int32, "i64": ctypes.c_int64, "f32": ctypes.c_float, "f64": ctypes.c_double}
_DTYPE = {"f32*": torch.float32, "i32*": torch.int32, "u8*": torch.uint8, "i64*": torch.int64, "f64*": torch.float64, "void*": None}
_RETURN = {"status": ctypes.c_int32, "i32": ctypes.c_int32, "i64": ctypes.c_int64, "str": ctypes.c_char_p}


def _ctype(kind):
    """Device pointers and the stream travel as integers (c_void_p); a host array as a pointer to its element type."""
    if kind in _SCALAR:
        return _SCALAR[kind]
    if kind[-1] != "]":
        return ctypes.c_void_p
    return ctypes.POINTER(_SCALAR.get(kind[:kind.index("[")], ctypes.c_void_p))


# the ctypes view of the table, {name: (restype, [argtypes])}: what load() installs (tools/ab_*.py install it on their own builds)
def _protos(signatures):
    return {name: (_RETURN[ret], [_ctype(k) for k in kinds]) for name, (ret, kinds) in signatures.items()}


_PROTOS = _protos(SIGNATURES)

# The small-network entries, one line per entry of include/nerf_mi355x_nn.h (the second header of the same library): the same kinds,
# the same parser.  tests/test_fused_mlp_cpu.py compares this table with that header as tests/test_abi_symbols.py does the core one.
_TABLE_NN = """
nerf_nn_abi_version  i32 :
nerf_fused_mlp_save_floats  i64 : i64 i32 i32
nerf_fused_mlp_grad_floats  i64 : i64 i32 i32 i32
nerf_fused_mlp_forward  status : f32* i64 i32 i32 i32 i32 i32 f32*[] f32*[] f32* f32* stream
nerf_fused_mlp_backward  status : f32* f32* f32* i64 i32 i32 i32 i32 i32 f32*[] f32* f32* f32*[] f32*[] f32* stream
nerf_sh4_encode  status : f32* i64 f32* stream
nerf_field_points  status : f32* f32* f32* i64 i64 i32 i32* i64 f32[3] f32[3] f32 f32* stream
nerf_field_color_inputs  status : f32* f32* i32* i64 i64 i32 f32* f32* stream
nerf_field_color_inputs_backward  status : f32* f32* i64 f32* stream
nerf_field_raw_scatter  status : f32* f32* i32* i64 i64 f32* stream
nerf_field_raw_gather  status : f32* i32* i64 i64 f32* f32* stream
"""
NN_SIGNATURES = _parse_table(_TABLE_NN)
NN_EXPORTS = tuple(NN_SIGNATURES)
_NN_PROTOS = _protos(NN_SIGNATURES)

# The spatial adjoint of the hash field's glue, one line per entry of include/nerf_mi355x_field.h (the third header of the same
# library; the second table is pinned at its 11 entries).  tests/test_hashfield_grad_cpu.py compares this table with that header.
_TABLE_FIELD = """
nerf_field_density_seed  status : f32* i64 i64 i32 f32* stream
nerf_field_points_backward  status : f32* f32* f32* i64 i64 i32 i32* i64 f32[3] f32[3] f32 f32* f32* i32 f32* f32* f32* stream
nerf_field_sh_gradient  status : f32* i32* i64 i64 i32 f32* stream
nerf_sh4_encode_backward  status : f32* f32* i64 f32* stream
"""
FIELD_SIGNATURES = _parse_table(_TABLE_FIELD)
FIELD_EXPORTS = tuple(FIELD_SIGNATURES)
_FIELD_PROTOS = _protos(FIELD_SIGNATURES)

# The deterministic table gradient of the hash-grid encoding, one line per entry of include/nerf_mi355x_hashgrid.h (the fourth header
# of the same library; the three tables above are pinned at their sizes).  tests/test_hashgrid_deterministic_cpu.py compares this
# table with that header.
_TABLE_HASHGRID = """
nerf_hashgrid_deterministic_workspace_bytes  i64 : i64 i32
nerf_hashgrid_deterministic_guard_bits  i32 : i64 i32
nerf_hashgrid_backward_deterministic  status : f32* f32* i64 i32 i32 i32 i32[] f32[] f32* void* i64 stream
"""
HASHGRID_SIGNATURES = _parse_table(_TABLE_HASHGRID)
HASHGRID_EXPORTS = tuple(HASHGRID_SIGNATURES)
_HASHGRID_PROTOS = _protos(HASHGRID_SIGNATURES)

# The exact weight and bias gradients of the fused MLP, one line per entry of include/nerf_mi355x_nn_exact.h (the fifth header of the
# same library; the four tables above are pinned at their sizes).  tests/test_fused_mlp_exact_cpu.py compares this table with that
# header.
_TABLE_NN_EXACT = """
nerf_fused_mlp_exact_workspace_bytes  i64 : i32 i32 i32 i32
nerf_fused_mlp_exact_guard_bits  i32 : i64
nerf_fused_mlp_backward_exact  status : f32* f32* f32* i64 i32 i32 i32 i32 i32 f32*[] f32* f32* f32*[] f32*[] f32* void* i64 stream
"""
NN_EXACT_SIGNATURES = _parse_table(_TABLE_NN_EXACT)
NN_EXACT_EXPORTS = tuple(NN_EXACT_SIGNATURES)
_NN_EXACT_PROTOS = _protos(NN_EXACT_SIGNATURES)

# The unit orders of the fp32 render MLP, one line per entry of include/nerf_mi355x_order.h (the sixth header of the same library; the
# five tables above are pinned at their sizes).  tests/test_unit_order_cpu.py compares this table with that header.  The matching is
# pure host: its two arrays are host arrays and its int32 status comes back unchecked (call() checks entries that take a stream).
_TABLE_ORDER = """
nerf_pack_model_ordered  status : f32*[24] u8* void* i32 stream
nerf_unit_order_stats  status : f32* i64 i32* stream
nerf_unit_order_match  i32 : i32[65536] i32[256]
"""
ORDER_SIGNATURES = _parse_table(_TABLE_ORDER)
ORDER_EXPORTS = tuple(ORDER_SIGNATURES)
_ORDER_PROTOS = _protos(ORDER_SIGNATURES)

# Where the samples of a hash-field ray lie, one line per entry of include/nerf_mi355x_sampling.h (one more header of the same library,
# next to nerf_mi355x_field.h; the six tables above are pinned at their sizes).  tests/test_hashfield_sampling_cpu.py compares this
# table with that header.
_TABLE_SAMPLING = """
nerf_field_sample_importance  status : f32* f32* i64 f32* i64 i64 i32 i32 f32* f32* stream
nerf_field_stratified_depths  status : f32* f32* i64 i32 f32* stream
nerf_field_density_scatter  status : f32* i64 i32* i64 i64 f32* stream
"""
SAMPLING_SIGNATURES = _parse_table(_TABLE_SAMPLING)
SAMPLING_EXPORTS = tuple(SAMPLING_SIGNATURES)
_SAMPLING_PROTOS = _protos(SAMPLING_SIGNATURES)

# The deformation field of a dynamic scene, one line per entry of include/nerf_mi355x_deform.h (one more header of the same library; the
# seven tables above are pinned at their sizes).  tests/test_deform_cpu.py compares this table with that header.  The two byte counts
# are pure host.
_TABLE_DEFORM = """
nerf_deform_packed_bytes  i64 : i32 i32 i32
nerf_deform_table_bytes  i64 : i32 i32 i32
nerf_deform_pack  status : f32*[3] i32 i32 i32 f32* stream
nerf_deform_unpack_grad  status : f32* i32 i32 i32 f32*[3] stream
nerf_deform_forward  status : f32* f32* i32* i64 i64 i32 f32* i32 i32 i32 f32* f32* stream
nerf_deform_backward  status : f32* f32* i32* i64 i64 i32 f32* i32 i32 i32 f32* f32* f32* stream
"""
DEFORM_SIGNATURES = _parse_table(_TABLE_DEFORM)
DEFORM_EXPORTS = tuple(DEFORM_SIGNATURES)
_DEFORM_PROTOS = _protos(DEFORM_SIGNATURES)

_lib = None


class NerfLibraryError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", CSRC], capture_output=True, text=True)
    if res.returncode != 0:
        raise NerfLibraryError("building libnerf_mi355x.so failed:\n" + res.stdout + res.stderr)
    if verbose:
        print(res.stdout)
    return LIB_PATH


def load():
    """dlopen the library and declare prototypes; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NerfLibraryError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()); "
                "there is no CPU fallback for the render path")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(_PROTOS.items()) + list(_NN_PROTOS.items()) + list(_FIELD_PROTOS.items()) +
                                  list(_HASHGRID_PROTOS.items()) + list(_NN_EXACT_PROTOS.items()) + list(_ORDER_PROTOS.items()) +
                                  list(_SAMPLING_PROTOS.items()) + list(_DEFORM_PROTOS.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.nerf_abi_version() != 3:
            raise NerfLibraryError("libnerf_mi355x.so ABI version mismatch")
        if lib.nerf_nn_abi_version() != 1:
            raise NerfLibraryError("libnerf_mi355x.so small-network ABI version mismatch (include/nerf_mi355x_nn.h)")
        if lib.nerf_build_flags() != 0:
            raise NerfLibraryError(f"{LIB_PATH} is a timing build (nerf_build_flags() = {lib.nerf_build_flags()}): kernels "
                                   "compiled with NERF_*_HACK_* switches compute wrong results; rebuild with `make -C csrc`")
        _lib = lib
    return _lib


class strided:
    """Marks a tensor argument of call() whose layout the caller has validated itself and describes to the entry with an explicit
    element stride (the `field` of nerf_isosurface_* and nerf_occupancy_build): dtype and device are checked, contiguity is not."""

    def __init__(self, tensor):
        self.tensor = tensor


def call(name, *args):
    """Call entry `name` of the library with `args` as its header lists them, minus the stream: tensors (None: NULL) for device
    pointers, numbers for scalars, sequences or ctypes arrays for host arrays.  Every argument is checked against the entry's kinds
    in SIGNATURES (or, looked up in this order, NN_SIGNATURES, FIELD_SIGNATURES, HASHGRID_SIGNATURES, NN_EXACT_SIGNATURES, ORDER_SIGNATURES,
    SAMPLING_SIGNATURES, DEFORM_SIGNATURES) before the library is touched; the work goes to the current torch stream of the tensors' device.  A status return
    is checked (NerfLibraryError with nerf_last_error's text); any other return value comes back as it is."""
    for table in (SIGNATURES, NN_SIGNATURES, FIELD_SIGNATURES, HASHGRID_SIGNATURES, NN_EXACT_SIGNATURES, ORDER_SIGNATURES,
                  SAMPLING_SIGNATURES, DEFORM_SIGNATURES):
        if name in table:
            break
    ret, kinds = table[name]
    has_stream = kinds[-1:] == ("stream",)
    if len(args) != len(kinds) - has_stream:
        raise TypeError(f"{name} takes {len(kinds) - has_stream} arguments ({len(args)} given)")
    dev = None

    def device_pointer(t, dtype, i):
        nonlocal dev
        if t is None:
            return None
        dense = not isinstance(t, strided)
        if not dense:
            t = t.tensor
        if not t.is_cuda:
            raise NerfLibraryError(f"{name}, argument {i}: the HIP render path needs tensors on a GPU (cuda) device; got a CPU tensor")
        if (dtype is not None and t.dtype != dtype) or (dense and not t.is_contiguous()):
            raise NerfLibraryError(f"{name}, argument {i}: expected a contiguous {dtype or 'byte'} tensor, got {t.dtype} with "
                                   f"strides {tuple(t.stride())}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise NerfLibraryError(f"{name}, argument {i}: a tensor on {t.device}, the earlier ones on {dev}")
        return t.data_ptr()

    cargs = []
    for i, (kind, a) in enumerate(zip(kinds, args)):
        if kind in _DTYPE:
            a = device_pointer(a, _DTYPE[kind], i)
        elif kind not in _SCALAR and a is not None:                 # a host array
            elem, _, length = kind[:-1].partition("[")
            if length and len(a) != int(length):
                raise NerfLibraryError(f"{name}, argument {i}: a host array of {length} is needed, got {len(a)}")
            if elem in _DTYPE:
                a = (ctypes.c_void_p * len(a))(*[device_pointer(t, _DTYPE[elem], i) for t in a])
            elif not isinstance(a, ctypes.Array):
                a = (_SCALAR[elem] * len(a))(*a)
        cargs.append(a)
    fn = getattr(load(), name)
    if not has_stream:
        return fn(*cargs)
    if dev is None or dev.index == torch.cuda.current_device():
        rc = fn(*cargs, None if dev is None else torch.cuda.current_stream(dev).cuda_stream)
    else:
        with torch.cuda.device(dev):
            rc = fn(*cargs, torch.cuda.current_stream(dev).cuda_stream)
    if ret == "status":
        check(rc, name)
    return rc


# The helpers below are the direct path to the C ABI: load() plus check / ptr / ptr_array / stream_of at the call site.  The package
# itself and the tests go through call(); bench.py, tools/ and the tests' refusal probes (which need the raw status of deliberately
# malformed arguments) call entries directly through these, so they stay.
def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().nerf_last_error().decode("utf-8", "replace")
        raise NerfLibraryError(f"{what or 'nerf call'} failed (status {rc}): {msg}")


def ptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA tensor of `dtype` (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NerfLibraryError("the HIP render path needs tensors on a GPU (cuda) device; got a CPU tensor")
    if t.dtype != dtype or not t.is_contiguous():
        raise NerfLibraryError(f"expected a contiguous {dtype} tensor")
    return t.data_ptr()


def ptr_array(tensors, dtype=None):
    """ctypes array of the device pointers of `tensors`; with `dtype`, each one checked as by ptr()."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if dtype is None else ptr(t, dtype) for t in tensors])


def zeroed_grads(params, device):
    """One fp32 gradient tensor per parameter, in order, as views of one zeroed buffer: one memset instead of one per tensor, and
    the layout dist.allreduce_gradients reduces in place."""
    flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=device)
    grads, off = [], 0
    for p in params:
        grads.append(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    return grads


def stream_of(device):
    return torch.cuda.current_stream(device).cuda_stream


def packed_model_bytes(precision: int) -> int:
    n = int(load().nerf_packed_model_bytes(precision))
    if n <= 0:
        raise NerfLibraryError(f"unknown precision {precision}")
    return n
