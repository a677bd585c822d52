"""What the host layer holds outside the graph's arenas is given back: p3d_debug_private_resources counts the device blocks, their
bytes and the timing events that are live in the process, and every facility that is closed -- and a session that is destroyed
with everything left open -- returns the counts to where they stood.  Exact integers; nothing is measured."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(batch=2, frames=16, height=32, width=32, base=16, blocks=(1, 1, 1))


def resources():
    from sap3d_tensorflow_amd import _lib
    b, n, e = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().p3d_debug_private_resources(C.byref(b), C.byref(n), C.byref(e)))
    return b.value, n.value, e.value


@pytest.fixture
def sess():
    from sap3d_tensorflow_amd import P3DSession
    gc.collect()          # a session another test dropped must not give its stores back in the middle of this one
    s = P3DSession("unet", seed=2, **SMALL)
    yield s
    s.close()


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def use_video(s, frames=16):
    """open, keep_source, 16 frames put as uint8 at 8 x 8, one predict, one read of the maps"""
    s.open_video(frames)
    s.video_keep_source(True)
    s.video_put_u8(0, _u8((frames, 8, 8, 3), 1))
    s.video_predict([0])
    s.video_maps(0, 16)


def use_trainset(s):
    s.open_trainset([16])
    s.trainset_put_frames_u8(0, 0, _u8((16, 32, 32, 3), 2))
    s.trainset_put_density_u8(0, 0, _u8((16, 8, 8), 3))
    s.trainset_stage([(0, 0), (0, 0)])


def use_prior(s):
    m = np.zeros((1, 8, 8), np.uint8)
    m[0, 2, 3] = 255
    s.open_prior((8, 8))
    s.prior_add(m)
    s.finish_prior()


def use_fixpool(s):
    m = np.zeros((2, 8, 8), np.uint8)
    m[0, 1, 1] = m[1, 5, 6] = 255
    s.open_fixation_pool((8, 8), 2)
    s.fixation_pool_put(0, m)
    s.shuffled_begin([[0, 1], [1, 0]])


def test_video_cycle(sess):
    base = resources()
    use_video(sess)
    blocks, nbytes, events = resources()
    # frames, maps, counts, the three per-call tables, the source store; the four events around gather and scatter
    assert blocks == base[0] + 7 and events == base[2] + 4
    assert nbytes == base[1] + 16 * (32 * 32 * 3 * 4 + 32 * 32 * 4 + 4) + 2 * 16 * (16 + 4) + 2 * 4 + 16 * 8 * 8 * 3
    sess.close_video()
    assert resources() == base          # p3d_video_close keeps nothing


def test_trainset_cycle(sess):
    base = resources()
    use_trainset(sess)
    blocks, nbytes, events = resources()
    # frames (bytes), densities, the staging buffer of the density put, the per-call table; the two events around the stage
    assert blocks == base[0] + 4 and events == base[2] + 2
    assert nbytes == base[1] + 16 * 32 * 32 * 3 + 16 * 32 * 32 + 16 * 8 * 8 + 2 * 4
    sess.close_trainset()
    assert resources() == base          # p3d_trainset_close keeps nothing


def test_prior_cycle(sess):
    base = resources()
    use_prior(sess)
    # counts, flag, staging; the finished map.  (the events of add and finish live for their call only)
    assert resources() == (base[0] + 4, base[1] + 8 * 8 * 4 + 4 + 8 * 8 + 8 * 8 * 4, base[2])
    sess.close_prior()
    # p3d_prior_close frees the accumulator; the finished prior is documented to stay, until it is replaced or dropped
    assert resources() == (base[0] + 1, base[1] + 8 * 8 * 4, base[2])
    sess.set_prior_map(np.arange(64, dtype=np.float32).reshape(8, 8))
    assert resources() == (base[0] + 1, base[1] + 8 * 8 * 4, base[2])
    sess.set_prior_map(None)
    assert resources() == base


def test_fixpool_cycle(sess):
    base = resources()
    use_fixpool(sess)
    blocks, nbytes, events = resources()
    assert blocks == base[0] + 2 + 6 and events == base[2]          # words, staging; the six buffers of the batch's union
    assert nbytes > base[1]
    sess.close_fixation_pool()
    assert resources() == base          # p3d_fixpool_close keeps nothing, the union included


def test_video_reopen_keeps_capacity(sess):
    base = resources()
    sess.open_video(32)
    big = resources()
    assert big[1] == base[1] + 32 * (32 * 32 * 3 * 4 + 32 * 32 * 4 + 4) + 2 * 16 * (16 + 4) + 2 * 4
    sess.open_video(16)                 # no close in between: the stores are large enough and stay
    assert resources() == big
    use_video(sess, 32)                 # the source store comes, and goes with the next open
    sess.open_video(16)
    assert resources() == big
    sess.close_video()
    assert resources() == base


def test_session_destruction_returns_everything():
    from sap3d_tensorflow_amd import P3DSession
    gc.collect()
    before = resources()
    s = P3DSession("unet", seed=2, **SMALL)
    use_video(s)
    use_trainset(s)
    use_prior(s)
    use_fixpool(s)
    held = resources()
    assert held[0] == before[0] + 7 + 4 + 4 + 8 and held[1] > before[1] and held[2] == before[2] + 4 + 2
    s.close()
    assert resources() == before


def test_op_level_hooks_hold_nothing():
    from sap3d_tensorflow_amd import _lib, ops
    from sap3d_tensorflow_amd._lib import check, fptr
    gc.collect()
    rng = np.random.default_rng(5)
    before = resources()
    ops.bias_add_grad(rng.standard_normal((4, 8)).astype(np.float32))
    assert resources() == before
    a, b = rng.random((1, 8), dtype=np.float32), rng.random((1, 8), dtype=np.float32)
    out = np.empty(1, np.float64)
    check(_lib.lib().p3d_metric_cc(0, fptr(a), fptr(b), 1, 8, out.ctypes.data_as(_lib._dp)))
    assert np.isfinite(out[0]) and resources() == before
