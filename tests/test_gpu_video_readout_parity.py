"""The read-outs of a resident video that end in bytes (P3DSession.video_maps_u8, video_score, video_score_auc, video_render,
video_reframe) share their preconditions and one stage interface: every shared refusal names its caller and changes nothing; the
AUC call without a sweep is video_score; the chain's second chunk reaches the scores, the images and the windows; and the smallest
shapes score as metrics.score_bytes scores them, render and reframe as their replays do."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as FR        # noqa: E402
import render_ref as RR         # noqa: E402
import score_u8_ref as R        # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SIZE, N_REP = 20, 16, (48, 40), 5
ALL = ("cc", "sim", "judd", "kl", "nss")


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _frames(F, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.5, (F, 32, 32, 3)).astype(np.float32)


def _truth(F, size=SIZE, seed=3):
    rng = np.random.default_rng(seed)
    den = R.blobs(rng, F, *size)
    fix = np.stack([R.fixations(rng, d, 40) for d in den])
    return den, fix


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _read(sess, reader, first, n, den, fix):
    from sap3d_tensorflow_amd import metrics
    if reader == "video_maps_u8":
        return sess.video_maps_u8(first, n, size=SIZE)
    if reader == "video_score":
        return sess.video_score(first, n, den[:n], fix[:n], size=SIZE)
    if reader == "video_render":
        return sess.video_render(first, n, frames=np.zeros((n,) + SIZE + (3,), np.uint8), size=SIZE)
    if reader == "video_reframe":
        return sess.video_reframe(first, n, (10, 8), frames=np.zeros((n,) + SIZE + (3,), np.uint8), size=SIZE)
    bidx, _ = metrics.borji_draws_u8(fix[:n], N_REP, np.random.RandomState(0))
    return sess.video_score_auc(first, n, den[:n], fix[:n], size=SIZE, borji_idx=bidx, n_rep=N_REP)


@pytest.mark.parametrize("reader", ["video_maps_u8", "video_score", "video_score_auc", "video_render", "video_reframe"])
def test_shared_preconditions_name_their_caller_and_change_nothing(reader):
    from sap3d_tensorflow_amd import P3dError
    sess = _session()
    den, fix = _truth(F20)

    def refused(text, first, n):
        with pytest.raises(P3dError, match=re.escape(text)):
            _read(sess, reader, first, n, den, fix)

    refused(reader + ": no video is open (p3d_video_open)", 0, 1)
    sess.open_video(F20, "mean")
    sess.video_put(0, _frames(F20, seed=6))
    sess.video_predict([0, 2])                        # frames 18 and 19 have no prediction
    before, info = sess.video_maps_u8(0, 18, size=SIZE), sess.video_info()
    refused(reader + ": frames 18 .. 21 are outside [0, 20)", 18, 4)
    refused(reader + ": frame 18 has no prediction yet (count 0)", 10, 10)
    sess.set_video_temporal("gauss", 1.0, 1, 0.0)     # frame 17 needs frame 18
    refused(reader + ": the temporal filter needs frame 18, which has no prediction yet (count 0)", 10, 8)
    sess.set_video_temporal("off")
    sess.set_hist_match("density")
    refused("hist_match: P3D_MATCH_DENSITY matches to a ground-truth density and runs in p3d_eval_last_frames only; written maps take "
            "P3D_MATCH_TABLE", 0, 4)
    sess.set_hist_match("off")
    assert sess.video_info() == info and np.array_equal(sess.video_maps_u8(0, 18, size=SIZE), before)
    sess.close_video()
    sess.close()


@pytest.fixture(scope="module")
def video():
    """A session whose 20-frame video is predicted throughout (mode "mean", windows 0 .. 4)."""
    sess = _session()
    sess.open_video(F20, "mean")
    sess.video_put(0, _frames(F20, seed=4))
    for i in range(0, 5, 3):
        sess.video_predict(list(range(5))[i:i + 3])
    yield sess
    sess.close_video()
    sess.close()


def test_columns_alone_through_the_auc_call_are_video_score(video):
    den, fix = _truth(F20)
    want = video.video_score(0, F20, den, fix, size=SIZE, columns=ALL)
    got = video.video_score_auc(0, F20, den, fix, size=SIZE, columns=ALL, borji_idx=None, shuffled_ranks=None, n_rep=N_REP)
    assert np.isfinite(want).all() and np.array_equal(_bits(got["scores"]), _bits(want))
    assert set(video.last_score_ms) == {"upload", "device", "score", "auc"} and video.last_score_ms["auc"] == 0.0
    assert got["borji"].shape == got["shuffled"].shape == (F20, N_REP)
    assert np.isnan(got["borji"]).all() and np.isnan(got["shuffled"]).all()


def test_the_second_chunk_of_the_chain_reaches_the_scores(video):
    from sap3d_tensorflow_amd import metrics
    den, fix = _truth(17)
    video.set_postprocess(1.5, 0, "range")            # the float32 chain: 16 maps, then 1
    try:
        got, maps = video.video_score(2, 17, den, fix, size=SIZE, columns=ALL, with_maps=True)
        assert np.array_equal(maps, video.video_maps_u8(2, 17, size=SIZE))
        assert len(np.unique(maps[16])) > 1           # (the last map is a map)
        assert np.array_equal(_bits(got), _bits(metrics.score_bytes(maps, den, fix, flags=ALL)))
    finally:
        video.set_postprocess(None)


@pytest.mark.parametrize("n,size", [(1, SIZE), (1, (1, 1)), (F20, (1, 1)), (F20, (7, 19))])
def test_degenerate_sizes_score_as_score_bytes(video, n, size):
    from sap3d_tensorflow_amd import metrics
    den, fix = _truth(n, size, seed=5)
    fix[::2] = 0                                      # every other map without fixation: NaN in AUC_Judd and NSS
    got, maps = video.video_score(0, n, den, fix, size=size, columns=ALL, with_maps=True)
    assert maps.shape == (n,) + size
    op = metrics.score_bytes(maps, den, fix, flags=ALL)
    assert np.array_equal(_bits(got), _bits(op))
    want = R.score_maps(maps, den, fix, R.ALL, R.EXPECTED)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    worst = max([R.rel(g, w) for g, w in zip(got.ravel(), want.ravel()) if not np.isnan(w)] or [0.0])
    print(n, size, "largest relative error", worst)
    assert worst <= R.GPU_GATE


CONTOUR = dict(contour=100, thickness=2, contour_color=(9, 8, 7))      # (R, G, B); the replay takes (B, G, R)


def test_the_second_chunk_of_the_chain_reaches_render_and_reframe(video):
    """Under the float32 chain (16 maps, then 1) the stage's bytes are video_maps_u8's, and what it makes of them is byte for byte
    what the op-level entries make of them; the track's filter (2 frames either side) crosses the chunk boundary."""
    from sap3d_tensorflow_amd import dataflow
    fr = RR.frames_for(np.zeros((17,) + SIZE, np.uint8))
    table = dataflow.render_table("jet", 0.6, "ramp", gate=30)
    video.set_postprocess(1.5, 0, "range")
    try:
        want = video.video_maps_u8(2, 17, size=SIZE)
        assert len(np.unique(want[16])) > 1           # (the last map is a map)
        img, maps = video.video_render(2, 17, frames=fr, size=SIZE, table=table, with_maps=True, **CONTOUR)
        assert np.array_equal(maps, want)
        assert np.array_equal(img, dataflow.render_overlay(maps, fr, table, **CONTOUR))
        got = video.video_reframe(2, 17, (10, 8), frames=fr, size=SIZE, gate=40, smooth=2, with_raw=True, with_mass=True, with_maps=True)
        assert np.array_equal(got["maps"], want)
        track, raw, mass, crop = dataflow.reframe(want, fr, (10, 8), gate=40, smooth=2)
        assert np.array_equal(got["raw"], raw) and np.array_equal(got["track"], track) and np.array_equal(got["mass"], mass)
        assert crop.shape == (17, 10, 8, 3) and np.array_equal(got["crop"], crop)
    finally:
        video.set_postprocess(None)


@pytest.mark.parametrize("n,size,crop", [(1, SIZE, (10, 8)), (F20, (1, 1), (1, 1)), (F20, (7, 19), (7, 1))])
def test_degenerate_sizes_render_and_reframe_as_their_replays(video, n, size, crop):
    from sap3d_tensorflow_amd import dataflow
    fr = RR.frames_for(np.zeros((n,) + size, np.uint8), seed=7)
    table = dataflow.render_table("hot", 0.5, "constant", gate=10)
    img, maps = video.video_render(0, n, frames=fr, size=size, table=table, with_maps=True, **CONTOUR)
    assert maps.shape == (n,) + size and img.shape == (n,) + size + (3,)
    assert np.array_equal(img, RR.render(maps, fr, table, 100, 2, (7, 8, 9)))
    got = video.video_reframe(0, n, crop, frames=fr, size=size, gate=20, smooth=1, with_raw=True, with_mass=True, with_maps=True)
    assert np.array_equal(got["maps"], maps)
    track, raw, mass, win = FR.reframe(maps, fr, crop[0], crop[1], 20, 1)
    assert np.array_equal(got["raw"], raw) and np.array_equal(got["track"], track) and np.array_equal(got["mass"], mass)
    assert got["crop"].shape == (n,) + crop + (3,) and np.array_equal(got["crop"], win)
