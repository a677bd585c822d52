"""P3DSession.video_detect_transitions / video_shot_kinds on a resident video made of tests/transitions_ref.py's planted video: the
signals, the table and the kinds are the replay's; under the installed table the temporal filter and the reframe track are
tests/shots_ref.py's, bit for bit; video_detect_shots afterwards returns what it returned before; refusals change nothing."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shots_ref as S          # noqa: E402
import temporal_ref as TR      # noqa: E402
import transitions_ref as T    # noqa: E402

CFG = dict(base=16, blocks=(1, 1, 1))
SRC, CROP, WIN = (24, 40), (24, 14), 16
F = T.FIXTURE_FRAMES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def video():
    """The session with the planted video resident and every frame predicted, its frames, and the replay's signals."""
    from sap3d_tensorflow_amd import P3DSession
    bgr = T.fixture(*SRC)
    sess = P3DSession("unet", seed=2, batch=4, frames=WIN, height=32, width=32, **CFG)
    sess.open_video(F, "newest")
    sess.video_keep_source(True)
    for i in range(0, F, 100):
        sess.video_put_u8(i, bgr[i:i + 100])
    starts = list(range(0, F - WIN, WIN)) + [F - WIN]
    for i in range(0, len(starts), 4):
        sess.video_predict(starts[i:i + 4])
    yield sess, bgr, T.signals(bgr, *T.FIXTURE_GRID, 12)
    sess.close_video()
    sess.close()


def test_detect_gives_the_replays_table_and_kinds(video):
    sess, bgr, (D, E, v) = video
    sess.video_set_shots(None)
    cuts_before = sess.video_detect_shots(T.FIXTURE_GRID, install=False, **T.FIXTURE_RULE)
    assert cuts_before.tolist() == T.FIXTURE_OFF_STARTS and sess.video_shots() is None and sess.video_shot_kinds() is None
    got = sess.video_detect_transitions(T.FIXTURE_GRID, install=False, with_signals=True, **T.FIXTURE_RULE, **T.GRADUAL_DEFAULTS)
    assert got[0].tolist() == T.FIXTURE_STARTS and got[1].tolist() == T.FIXTURE_KINDS
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[2], D) and np.array_equal(got[3], E) and np.array_equal(got[4], v) and got[4].dtype == np.int64
    assert sess.video_shots() is None                        # nothing is installed unless asked for
    ms = sess.video_shots_last_ms()
    assert ms["signal"] > 0.0 and ms["decision"] > 0.0
    # another grid and lag; dissolves or fades off; both off: the cut table
    for grid, gradual in (((2, 3), dict(T.GRADUAL_DEFAULTS, lag=20)), ((1, 1), dict(T.GRADUAL_DEFAULTS, lag=0)), ((4, 4), dict(T.GRADUAL_DEFAULTS, mono_min=0)),
                          ((4, 4), dict(T.GRADUAL_DEFAULTS, lag=0, mono_min=0))):
        sig = T.signals(bgr, *grid, gradual["lag"])
        starts, kinds = sess.video_detect_transitions(grid, install=False, **T.FIXTURE_RULE, **gradual)
        assert (starts.tolist(), kinds.tolist()) == T.transitions(*sig, SRC[0] * SRC[1], T.FIXTURE_RULE, gradual), (grid, gradual)
    assert starts.tolist() == T.FIXTURE_OFF_STARTS
    # installed: the table and its kinds; a table from elsewhere reports cuts
    starts, kinds = sess.video_detect_transitions(T.FIXTURE_GRID, **T.FIXTURE_RULE, **T.GRADUAL_DEFAULTS)
    assert sess.video_shots().tolist() == T.FIXTURE_STARTS and sess.video_shot_kinds().tolist() == T.FIXTURE_KINDS
    assert sess.video_detect_shots(T.FIXTURE_GRID, install=False, **T.FIXTURE_RULE).tolist() == cuts_before.tolist()
    assert sess.video_shots().tolist() == T.FIXTURE_STARTS and sess.video_shot_kinds().tolist() == T.FIXTURE_KINDS
    assert sess.video_detect_shots(T.FIXTURE_GRID, **T.FIXTURE_RULE).tolist() == T.FIXTURE_OFF_STARTS
    assert sess.video_shot_kinds().tolist() == [T.FIRST, T.CUT, T.CUT]
    sess.video_detect_transitions(T.FIXTURE_GRID, **T.FIXTURE_RULE, **T.GRADUAL_DEFAULTS)
    sess.video_set_shots([0, 5, 9, 100])
    assert sess.video_shot_kinds().tolist() == [T.FIRST, T.CUT, T.CUT, T.CUT]
    sess.video_set_shots(None)
    assert sess.video_shot_kinds() is None


@pytest.mark.parametrize("kind", ["gauss", "ema"])
def test_the_temporal_filter_stays_inside_the_found_shots(video, kind):
    sess, _, _ = video
    sess.video_set_shots(None)
    sess.set_video_temporal("off", 0., 0, 0.)
    plain = sess.video_maps(0, F)
    args = ("gauss", 1.5, 3, 0.0) if kind == "gauss" else ("ema", 0., 0, 0.7)
    sess.set_video_temporal(*args)
    no_table = sess.video_maps(0, F)
    sess.video_detect_transitions(T.FIXTURE_GRID, **T.FIXTURE_RULE, **T.GRADUAL_DEFAULTS)
    want = S.temporal_shots(TR.parse(TR.KINDS[args[0]], *args[1:]), plain, T.FIXTURE_STARTS)
    got = sess.video_maps(0, F)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got[20:30]), bits(no_table[20:30]))       # the dissolve at 24 now ends a shot
    sess.set_video_temporal("off", 0., 0, 0.)
    sess.video_set_shots(None)


def test_the_reframe_track_stays_inside_the_found_shots(video):
    sess, bgr, _ = video
    sess.video_set_shots(None)
    sess.set_video_temporal("off", 0., 0, 0.)
    sess.video_detect_transitions(T.FIXTURE_GRID, **T.FIXTURE_RULE, **T.GRADUAL_DEFAULTS)
    res = sess.video_reframe(0, F, CROP, gate=10, smooth=3, with_raw=True, with_mass=True, with_maps=True)
    track, raw, mass, crop = S.reframe_shots(res["maps"], bgr, *CROP, 10, 3, T.FIXTURE_STARTS)
    assert np.array_equal(res["raw"], raw) and np.array_equal(res["mass"], mass) and np.array_equal(res["crop"], crop)
    assert np.array_equal(res["track"], track)
    sess.video_set_shots(None)


def test_refusals_change_nothing(video):
    from sap3d_tensorflow_amd import P3dError
    sess, _, _ = video
    sess.video_set_shots([0, 7])
    for kw, word in ((dict(grid=(5, 1)), "grid"), (dict(threshold=0), "threshold"), (dict(min_length=0), "minimum length"), (dict(lag=1), "lag"),
                     (dict(lag=65), "lag"), (dict(high=0), "high"), (dict(dip=257), "dip"), (dict(mono=65536), "mono"), (dict(mono_min=-1), "mono_min")):
        args = dict(T.FIXTURE_RULE, grid=T.FIXTURE_GRID, **T.GRADUAL_DEFAULTS)
        args.update(kw)
        with pytest.raises(P3dError) as e:
            sess.video_detect_transitions(**args)
        assert word in str(e.value), kw
        assert sess.video_shots().tolist() == [0, 7] and sess.video_shot_kinds().tolist() == [T.FIRST, T.CUT]
    sess.video_set_shots(None)
