"""No-GPU checks of the resident training set's host side: the clip list of the reference's VideoDataset.setup_video_dataset_p3d
(dataflow.py:39-62), the seeded split, and the numpy replay's closed forms (tests/trainset_ref.py) against the oracle's numpy port
of `mapf`."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trainset_ref as tr        # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_clip_tuples_is_the_references_list():
    from sap3d_tensorflow_amd.dataflow import clip_tuples
    assert clip_tuples([30, 27, 40], 16, overlap=8, skip_head=11) == [(0, 11), (1, 11), (2, 11), (2, 19)]
    # the defaults: step 1 from frame 11, the last clip ending on the last frame; a video too short for one clip gives none
    assert clip_tuples([30, 26]) == [(0, j) for j in range(11, 15)]
    assert clip_tuples([16], 16, overlap=0, skip_head=0) == [(0, 0)]
    assert clip_tuples([], 16) == []


@pytest.mark.parametrize("overlap", [16, 17])
def test_an_overlap_of_a_whole_clip_is_refused(overlap):
    from sap3d_tensorflow_amd.dataflow import clip_tuples
    with pytest.raises(ValueError):
        clip_tuples([40], 16, overlap=overlap)


def test_split_clips_is_a_reproducible_partition():
    from sap3d_tensorflow_amd.dataflow import clip_tuples, split_clips
    tuples = clip_tuples([60, 45, 80], 16, overlap=13)
    n = len(tuples)
    assert n > 20
    for props in (0.0, 0.3, 0.8, 0.99, 1.0):
        train, valid = split_clips(tuples, props, np.random.default_rng(5))
        assert len(train) == int(n * props) and len(valid) == n - len(train)
        assert sorted(train + valid) == sorted(tuples)
        again = split_clips(tuples, props, np.random.default_rng(5))
        assert again == (train, valid)
        assert split_clips(tuples, props, 5) == (train, valid)              # a seed stands for its Generator
    a, _ = split_clips(tuples, 0.8, np.random.default_rng(5))
    b, _ = split_clips(tuples, 0.8, np.random.default_rng(6))
    assert a != b and a != tuples[:len(a)]


def test_u8_closed_form_equals_the_oracles_mapf_at_grid_size():
    """For a frame decoded at the grid's size every resize weight of mapf is 0; the replay's fsub / fdiv must give the oracle's
    bits, also where byte == mean (+0, never -0) and one below it."""
    from oracle import dataflow as od
    mean = od.MEAN_RGB                                   # (90, 102, 98): every byte value meets it, and its neighbours, below
    H, W = 16, 48
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    bgr[0, :, :] = np.arange(W)[:, None] + 70            # 70 .. 117 in every channel: 89, 90, 91, 97 .. 103
    bgr[1, :256 // 8, 0] = 255
    bgr[2].reshape(-1)[:] = np.resize(np.arange(256), W * 3)
    want = od.mapf_frame(bgr, H, W)
    got = tr.normalise_u8(bgr, mean)
    assert np.array_equal(bits(got), bits(want))
    zero = got[0, :, 0][bgr[0, :, 2] == 90]              # R == its mean
    assert zero.size == 1 and bits(zero)[0] == 0         # +0
    below = got[0, :, 0][bgr[0, :, 2] == 89]
    assert below.size == 1 and below[0] < 0 and bits(below)[0] == bits(np.float32(-1.0) / np.float32(255.0))


def test_u8_closed_form_with_means_that_are_no_integers():
    from oracle import dataflow as od
    mean = np.array([90.25, 101.7, 98.3], np.float32)
    bgr = np.random.default_rng(1).integers(0, 256, (7, 5, 3)).astype(np.uint8)
    im = bgr[:, :, ::-1].astype(np.float32) - mean[None, None, :]
    want = (od.resize_linear(im, 7, 5) / np.float32(255.0)).astype(np.float32)
    assert np.array_equal(bits(tr.normalise_u8(bgr, mean)), bits(want))


def test_density_closed_form_equals_the_oracle():
    from oracle import dataflow as od
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(bits(tr.density_f32(grey)), bits(od.mapf_density(grey, 16, 16)))
    src = np.random.default_rng(2).integers(0, 256, (48, 40)).astype(np.uint8)
    assert np.array_equal(bits(tr.density_f32(od.resize_linear_u8(src, 32, 32))), bits(od.mapf_density(src, 32, 32)))


def test_replay_cuts_clips_of_concatenated_videos():
    frames = [3, 5, 9]
    T = 3
    store = np.arange(17 * 2, dtype=np.uint8).reshape(17, 2)
    clips = [(0, 0), (2, 6), (2, 5), (1, 1)]
    assert tr.clip_first_frames(frames, clips, T) == [0, 14, 13, 4]
    got = tr.cut(store, frames, clips, T)
    assert got.shape == (4, 3, 2) and np.array_equal(got[1], store[14:17]) and np.array_equal(got[3], store[4:7])
    for bad in ([(0, 1)], [(1, 3)], [(3, 0)], [(2, -1)]):
        with pytest.raises(ValueError):
            tr.clip_first_frames(frames, bad, T)
