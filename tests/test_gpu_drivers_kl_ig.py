"""drivers/test.py --kldiv --info-gain BASELINE.npy end to end on synthetic clips: the two extra means on the final line, the
reference's line untouched without the flags, and a baseline of another shape refused before anything runs."""
import contextlib
import importlib.util
import io
import os

import numpy as np
import pytest

import kl_ig_ref as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(base=16, blocks=(2, 2, 3))
# test.py:182-183, as the driver printed it before the flags existed
ALL_LINE = " All: %d, Metrics: CC: %.3f  SIM: %.3f   NSS: %.3f  AUC_Judd: %.3f   AUC_Borji: %.3f"


def _driver():
    spec = importlib.util.spec_from_file_location("test_driver_kl_ig_gpu", os.path.join(ROOT, "drivers", "test.py"))
    d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d)
    return d


def _main(d, args):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cols = d.main(args)
    return cols, buf.getvalue().splitlines()


def test_driver_prints_the_two_extra_means(tmp_path):
    from sap3d_tensorflow_amd import P3DSession, synthetic
    d = _driver()
    s = P3DSession("unet", batch=2, seed=0, **CFG)
    s.init_params(7)
    s.save_checkpoint(str(tmp_path), 5)
    base = K.prior(1080, 960)
    np.save(str(tmp_path / "prior.npy"), base)
    args = ["--model", str(tmp_path), "--structure", "unet", "--base", "16", "--blocks", "2,2,3", "--batch", "2", "--clips", "4",
            "--seed", "3"]
    cols, lines = _main(d, args)
    assert len(cols) == 5
    c, sim, judd, borji, nss = [float(np.mean(np.asarray(v)[~np.isnan(v)])) for v in cols]
    plain = ALL_LINE % (2, c, sim, nss, judd, borji)
    assert [l for l in lines if l.startswith(" All:")] == [plain]
    assert not any("KLdiv" in l or "IG" in l for l in lines)
    # what the flags should add: the session's own extras on the same batches
    x, dens, fix = synthetic.synthetic_test_set(3, 4)
    s.set_eval_extra(kldiv=True, info_gain=True, baseline=base)
    np.random.seed(3)
    extras = []
    for lo in (0, 2):
        s.evaluate(x[lo:lo + 2], dens[lo:lo + 2], fix[lo:lo + 2])
        extras.append(s.last_eval_extra())
    extras = np.concatenate(extras)
    kl, ig = (float(np.mean(v[~np.isnan(v)])) for v in extras.T)
    cols7, lines = _main(d, args + ["--kldiv", "--info-gain", str(tmp_path / "prior.npy")])
    assert len(cols7) == 7 and np.array_equal(np.array(cols7[:5]), np.array(cols), equal_nan=True)
    assert np.array_equal(np.array(cols7[5:]).T, extras, equal_nan=True)
    assert [l for l in lines if l.startswith(" All:")] == [plain + "   KLdiv: %.3f   IG: %.3f" % (kl, ig)]
    cols6, lines = _main(d, args + ["--kldiv"])
    assert len(cols6) == 6 and [l for l in lines if l.startswith(" All:")] == [plain + "   KLdiv: %.3f" % kl]
    np.save(str(tmp_path / "small.npy"), K.prior(90, 80))
    with pytest.raises(ValueError, match="--info-gain"):
        d.main(args + ["--info-gain", str(tmp_path / "small.npy")])
    s.close()
