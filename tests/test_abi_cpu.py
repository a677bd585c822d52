"""No-GPU checks of the boundary: libp3dhip.so loads, exports every symbol include/p3d_hip.h declares, and
refuses loudly (no CPU fallback) when there is no HIP device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 30
    # the hooks of the attention block (tests/test_gpu_attention.py) are declared, exported and bound like every other symbol
    assert {"p3d_debug_attention_core", "p3d_debug_attention_splits", "p3d_debug_softmax_rows", "p3d_debug_attn_mix"} <= set(names)
    # ... and so are the hooks of the fused-BatchNorm launches (tests/test_gpu_fused_ops.py)
    assert {"p3d_debug_fused_conv", "p3d_debug_fused_wgrad", "p3d_debug_fused_reject"} <= set(names)
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, "ctypes signature missing for " + n


def test_malformed_fused_launches_are_refused_ahead_of_any_device_call():
    """p3d_debug_fused_reject: the launchers' argument checks run before the first HIP call, so they answer without a device too --
    hipErrorInvalidValue (1) for every malformed fused launch, and `false` from the filter-gradient validator for its three."""
    from sap3d_tensorflow_amd import ops
    for which in range(10):
        err, ok = ops.fused_reject(which)
        assert err == 1, (which, err)
        assert ok == (which < 7), which


def test_attention_plan_hook_needs_no_device():
    """p3d_debug_attention_splits is host only: the K-slice plans of the stored-score products are a function of the shapes."""
    from sap3d_tensorflow_amd import ops, P3dError
    assert ops.attention_splits(2, 300, 77, 32) == (1, 1, 1, 1)
    sp = ops.attention_splits(1, 8, 1024, 32)
    assert sp[0] == 1 and sp[1] > 1 and sp[2] == 1 and sp[3] > 1
    with pytest.raises(P3dError):
        ops.attention_splits(1, 8, 1024, 40)


def test_default_config_is_the_reference_architecture():
    from sap3d_tensorflow_amd import _lib
    cfg = _lib.P3dConfig()
    _lib.lib().p3d_default_config(C.byref(cfg))
    assert (cfg.structure, cfg.batch, cfg.frames, cfg.height, cfg.width, cfg.base) == (0, 2, 16, 112, 112, 64)
    assert list(cfg.blocks) == [3, 8, 36] and cfg.world_size == 1


def test_no_device_means_a_loud_error_not_a_fallback():
    from sap3d_tensorflow_amd import P3DSession, P3dError
    try:
        s = P3DSession("unet", batch=1, base=8, blocks=(1, 1, 1), frames=16, height=16, width=16)
    except P3dError as e:
        assert "device" in str(e).lower()          # "no ROCm-capable device is detected" / "no HIP device"
    else:
        s.close()                                  # GPU box: creating a session must simply work


def test_bad_arguments_raise():
    from sap3d_tensorflow_amd import P3DSession
    with pytest.raises(ValueError):
        P3DSession("unet++", batch=1)              # heads that are not built are named, not silently replaced


def test_gen_pred_driver_host_logic():
    """drivers/gen_pred.py: the sliding-window write-out rule (gen_pred.py:154-168) with a stand-in session
    (identity-like forward), no GPU.  (The frame pre-processing is a GPU kernel: tests/test_metrics.py.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)

    class Fake:
        def predict_windows(self, clips):
            return clips[..., :1] * 0 + clips[:, :, :1, :1, :1].mean(axis=4, keepdims=True)      # per-frame constant maps
    tag = np.arange(20, dtype=np.float32)[:, None, None, None] * np.ones((1, 112, 112, 3), np.float32)
    out = gp.predict_video(Fake(), tag, batch=3)
    assert np.allclose(out[:, 0, 0], np.arange(20))        # frame i's map comes from a window that contains frame i last (or window 0)


def test_product_synthetic_inputs_match_the_oracle_law():
    from oracle import p3d
    from sap3d_tensorflow_amd import synthetic
    assert np.array_equal(synthetic.synthetic_clip(3, (1, 16, 8, 8, 3)), p3d.synthetic_clip(3, (1, 16, 8, 8, 3)))
    assert np.array_equal(synthetic.synthetic_target(4, (1, 16, 8, 8)), p3d.synthetic_target(4, (1, 16, 8, 8)))


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under sap3d_tensorflow_amd/ or drivers/ may import it; bench.py may
    only inside cpu_baseline()."""
    import ast
    for d in ("sap3d_tensorflow_amd", "drivers"):
        for f in os.listdir(os.path.join(ROOT, d)):
            if f.endswith(".py"):
                src = open(os.path.join(ROOT, d, f)).read()
                assert "oracle" not in [n.split(".")[0] for node in ast.walk(ast.parse(src))
                                        for n in ([a.name for a in node.names] if isinstance(node, ast.Import) else
                                                  [node.module or ""] if isinstance(node, ast.ImportFrom) else [])], (d, f)
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    for fn in [n for n in tree.body if isinstance(n, ast.FunctionDef)]:
        uses = any(isinstance(n, ast.ImportFrom) and (n.module or "").startswith("oracle") for n in ast.walk(fn))
        assert (not uses) or fn.name == "cpu_baseline", fn.name


def test_no_floating_point_atomics_in_the_kernel_sources():
    """every cross-block sum is folded in a fixed order.  The only atomics allowed in csrc/ are integer
    ones (arrival tickets, the AUC histogram counters)."""
    import glob
    import re
    bad = []
    for f in sorted(glob.glob(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "*"))):
        for i, line in enumerate(open(f, errors="replace"), 1):
            code = line.split("//")[0]
            if "p.stamps" in code:          # the tools/micro-only cycle stamps (-DP3D_TUNE_STAMPS): 64-bit integer counters
                continue
            if re.search(r"unsafeAtomicAdd|atomicAdd\s*\(\s*(?!&cnt\[)|atomic_add_f|__hip_atomic_fetch_add\s*\([^,]*,\s*[^,]*[.f]", code):
                bad.append("%s:%d: %s" % (os.path.basename(f), i, line.strip()))
    assert not bad, bad


def test_product_build_reads_only_its_documented_environment():
    """The shipped library reads four environment variables ("Execution switches"); every tuning switch goes
    through p3d_tune_env, which a build without -DP3D_TUNING compiles to "not set" -- a stray P3D_TUNE_* variable in a
    training job cannot change results."""
    import glob
    import re
    direct, names = [], set()
    for f in sorted(glob.glob(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "*"))):
        for i, line in enumerate(open(f, errors="replace"), 1):
            code = line.split("//")[0]
            for m in re.finditer(r"(?<![_a-zA-Z])getenv\s*\(\s*(\"[A-Z0-9_]+\"|name)", code):
                direct.append("%s:%d" % (os.path.basename(f), i))
                if m.group(1) != "name":
                    names.add(m.group(1).strip('"'))
    assert len(direct) <= 6, direct
    assert names == {"P3D_DEBUG_SYNC", "P3D_GRAPH", "P3D_NO_SIDE_STREAM", "P3D_BUCKET_MB"}, names
    hdr = open(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "p3d_kernels.h")).read()
    body = hdr[hdr.index("p3d_tune_env"):]
    assert re.search(r"#if defined\(P3D_TUNING\)\s+return getenv\(name\);\s+#else", body), "p3d_tune_env must be compiled out of the product build"


def test_every_fill_and_copy_in_the_library_names_its_stream():
    """A bare hipMemset / hipMemcpy (/ 2D) runs on the null stream, which is not ordered against the handle's non-blocking
    streams: in rounds 3 and 4 such a call raced a launch (arrival counters zeroed under a running kernel; decision-hook
    scratch zeroed while its gate kernels ran).  Every fill / copy in csrc/ goes through the *Async form with an explicit
    stream (net.hip: fill_async, fill_now, copy_now); the allow-list is empty."""
    import glob
    import re
    bad = []
    for f in sorted(glob.glob(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "*"))):
        for i, line in enumerate(open(f, errors="replace"), 1):
            code = line.split("//")[0]
            if re.search(r"\bhipMem(set|cpy)(2D|3D)?\s*\(", code) or re.search(r"\bhipMemcpy(DtoH|HtoD|DtoD)\s*\(", code):
                bad.append("%s:%d: %s" % (os.path.basename(f), i, line.strip()))
    assert not bad, bad
