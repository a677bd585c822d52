"""ctypes binding of libp3dhip.so, read from include/p3d_hip.h (_header.py): every signature, structure layout and number
the header states comes from there.  There is no CPU fallback: a missing or unloadable library, or a box without a HIP
device, raises."""
import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3D_LIB: another build of the same library (same-box A/Bs against an older round's, tools/ab/); every declared symbol must
# still bind, so it cannot be anything else
LIB_PATH = os.environ.get("P3D_LIB") or os.path.join(_HERE, "libp3dhip.so")

_H = _header.read()          # parsed once, at import
# every symbol include/p3d_hip.h declares: name -> (restype, argtypes)
SIGNATURES = _H.functions
# every struct of the header under its class name, p3d_video_temporal -> P3dVideoTemporal: P3dConfig, P3dOpTime, P3dAugment,
# P3dPostprocess, P3dRender, P3dReframe, P3dVideoTemporal, P3dHistMatch, P3dFusedBn, P3dFusedBnGrad, P3dFusedGate, P3dFusedConv
globals().update((s.__name__, s) for s in _H.structs.values())
# the header's enumerators and integer #defines, each under its own name as well (P3D_COMM_ID_BYTES, P3D_LOSS_KLD_CC,
# P3D_LOSS_SALIENCY, P3D_PRIOR_MAX_MAPS, ...); the dicts below give them their Python-side names
K = _H.constants
globals().update(K)

# p3d_set_loss kinds
LOSSES = {"smooth_l1": K["P3D_LOSS_SMOOTH_L1"], "bce": K["P3D_LOSS_BCE"], "l1": K["P3D_LOSS_L1"]}
# the per-map loss P3D_LOSS_KLD_CC under its names: (kld_weight, cc_weight) of p3d_set_loss_weights
MAP_LOSSES = {"kld": (1.0, 0.0), "kld_cc": (1.0, 1.0)}
# the per-map loss with a fixation map, P3D_LOSS_SALIENCY: (kld, cc, nss, sim) of p3d_set_saliency_weights
SALIENCY_LOSSES = {"kld_cc_nss": (1.0, 1.0, 1.0, 0.0), "kld_cc_nss_sim": (1.0, 1.0, 1.0, 1.0)}
# p3d_set_regularization terms
REGULARIZATION = {"weightdecay": K["P3D_REG_WEIGHT_DECAY"], "l2": K["P3D_REG_L2"]}
# p3d_set_optimizer kinds and the TF slot names of each kind's slots 0, 1 (<var>/<suffix>)
OPTIMIZERS = {"adam": K["P3D_OPT_ADAM"], "momentum": K["P3D_OPT_MOMENTUM"], "sgd": K["P3D_OPT_SGD"]}
SLOT_NAMES = {"adam": ("Adam", "Adam_1"), "momentum": ("Momentum",), "sgd": ()}
# p3d_set_postprocess normalisations
NORMS = {"none": K["P3D_NORM_NONE"], "max": K["P3D_NORM_MAX"], "range": K["P3D_NORM_RANGE"]}
# p3d_set_hist_match modes
MATCH_MODES = {"off": K["P3D_MATCH_OFF"], "table": K["P3D_MATCH_TABLE"], "density": K["P3D_MATCH_DENSITY"]}
# p3d_set_eval_extra flags
EVAL_EXTRA = {"kldiv": K["P3D_EVAL_KLDIV"], "info_gain": K["P3D_EVAL_INFO_GAIN"]}
# p3d_video_open modes
VIDEO_MODES = {"newest": K["P3D_VIDEO_NEWEST"], "mean": K["P3D_VIDEO_MEAN"]}
# p3d_video_score / p3d_score_maps_u8: the columns' flags (also their order in a row of scores) and the AUC-Judd ties laws
SCORE_COLUMNS = {"cc": K["P3D_SCORE_CC"], "sim": K["P3D_SCORE_SIM"], "judd": K["P3D_SCORE_JUDD"], "kl": K["P3D_SCORE_KL"],
                 "nss": K["P3D_SCORE_NSS"]}
SCORE_MATLAB = ("cc", "sim", "judd")
SCORE_TIES = {"reference": K["P3D_SCORE_TIES_REFERENCE"], "expected": K["P3D_SCORE_TIES_EXPECTED"]}
# p3d_trainset_open frame formats
TRAINSET_FORMATS = {"u8": K["P3D_TRAINSET_FRAMES_U8"], "f32": K["P3D_TRAINSET_FRAMES_F32"]}
# dataflow.render_table: this project's own colour maps and the two opacity laws
RENDER_COLORMAPS = ("grey", "hot", "jet")
RENDER_OPACITIES = ("constant", "ramp")
# p3d_set_video_temporal kinds
TEMPORAL_KINDS = {"off": K["P3D_TEMPORAL_OFF"], "gauss": K["P3D_TEMPORAL_GAUSS"], "ema": K["P3D_TEMPORAL_EMA"]}
# what a map adds to the prior accumulator, and how the stage combines a map with the prior
PRIOR_KINDS = {"fixations": K["P3D_PRIOR_FIXATIONS"], "bytes": K["P3D_PRIOR_BYTES"]}
PRIOR_MODES = {"off": K["P3D_PRIOR_OFF"], "mul": K["P3D_PRIOR_MUL"], "mix": K["P3D_PRIOR_MIX"]}


class P3dError(RuntimeError):
    pass


_lib = None
# pointer types for the call sites' casts
_fp = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_ubyte)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)


def _torch_lib_dir():
    """Directory of the ROCm libraries a PyTorch-ROCm wheel bundles (torch/lib), or None.  Does not import torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        return None
    if spec is None or not spec.origin:
        return None
    d = os.path.join(os.path.dirname(spec.origin), "lib")
    return d if os.path.exists(os.path.join(d, "libamdhip64.so")) else None


def _one_rocm_runtime_per_process():
    """One HIP runtime per process, whatever the import order.  PyTorch-ROCm wheels bundle their own libamdhip64 /
    libhsa-runtime64 / librccl (torch/lib) under the same sonames as /opt/rocm's.  If libp3dhip.so were loaded first it
    would bind to /opt/rocm's copies, a later `import torch` would map the bundled ones next to them: two HIP runtimes
    in one process (tools/dupe_probe.py).  So when such a wheel is installed and torch is not loaded yet, its bundled runtime is mapped
    here BY PATH, without importing torch (a first `import torch` costs a minute or two on a fresh box): libp3dhip then
    binds to it by soname, and so does torch whenever it is imported.  With torch already imported nothing is needed."""
    import sys
    if "torch" in sys.modules:
        return
    if mapped_rocm_runtimes():
        return          # a runtime is already mapped (e.g. rocprofv3 preloads /opt/rocm's): bind to that one
    d = _torch_lib_dir()
    if d is None:
        return
    for name in ("libhsa-runtime64.so", "libamdhip64.so", "librccl.so"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            C.CDLL(p)        # RTLD_LOCAL: see lib()


def mapped_rocm_runtimes():
    """{library stem: sorted list of distinct files mapped into this process} for the HIP / HSA / RCCL runtimes."""
    import re
    found = {}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                m = re.search(r"(/\S*/(libamdhip64|libhsa-runtime64|librccl)\.so[^\s/]*)", line)
                if m:
                    found.setdefault(m.group(2), set()).add(os.path.realpath(m.group(1)))
    except OSError:
        pass
    return dict((k, sorted(v)) for k, v in found.items())


def _refuse_two_runtimes():
    dup = dict((k, v) for k, v in mapped_rocm_runtimes().items() if len(v) > 1)
    if dup:
        raise P3dError("two copies of a ROCm runtime library are mapped into this process (%s): it would crash at exit. "
                       "Load sap3d_tensorflow_amd (or torch) before anything else that pulls in a HIP runtime; see "
                       "INTEGRATION.md, 'One HIP runtime per process'." % dup)


_sessions = None


def register_session(s):
    """Sessions are closed, and the library's process-wide device resources released, from a Python atexit hook -- i.e.
    before interpreter finalisation and before any C++ static destructor -- so teardown never depends on the order in
    which libraries were loaded."""
    global _sessions
    if _sessions is None:
        import weakref
        _sessions = weakref.WeakSet()
    _sessions.add(s)


def _shutdown():
    if _sessions is not None:
        for s in list(_sessions):
            try:
                s.close()
            except Exception:
                pass
    if _lib is not None:
        try:
            _lib.p3d_shutdown()
        except Exception:
            pass


def lib():
    """Load libp3dhip.so once.  Raises if it has not been built (python -m sap3d_tensorflow_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P3dError("libp3dhip.so is not built (%s); run `python sap3d_tensorflow_amd/build.py`. "
                           "There is no CPU fallback." % LIB_PATH)
        _one_rocm_runtime_per_process()
        # RTLD_LOCAL (ctypes' default), never RTLD_GLOBAL: with its symbols in the global scope a later `import torch`
        # binds some of torch's C++ runtime symbols to this library's copies and the process dies at interpreter exit
        # (`double free or corruption`), even with a single HIP runtime mapped (tests/test_load_order.py)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _refuse_two_runtimes()
        _lib = l
        import atexit
        atexit.register(_shutdown)
    return _lib


def check(rc):
    if rc != 0:
        raise P3dError(lib().p3d_last_error().decode("utf-8", "replace"))


def fptr(a):
    return a.ctypes.data_as(_fp) if a is not None else None
