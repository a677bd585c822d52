"""drivers/gen_pred.py's ChunkWriter, the one place where a chunk of images is encoded on threads while the device runs the next:
every frame is written once, a writer's exception reaches the caller, and a chunk is submitted only once the one before it is done."""
import importlib.util
import os
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = [(0, 16), (16, 16), (32, 5)]


def _driver():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def _images(first, n):
    return np.arange(first, first + n, dtype=np.uint8)[:, None, None] * np.ones((1, 3, 2), np.uint8)


def test_every_frame_is_written_once_with_its_own_image():
    gp = _driver()
    seen, lock = [], threading.Lock()

    def write_one(f, m):
        with lock:
            seen.append((f, m.copy()))

    with gp.ChunkWriter(3, write_one) as w:
        for first, n in CHUNKS:
            w.hand_over(range(first, first + n), _images(first, n))
    assert sorted(f for f, _ in seen) == list(range(37))
    assert all(m.shape == (3, 2) and (m == f).all() for f, m in seen)
    assert w.encode_ms >= 0.0 and not w.held


def test_frame_indices_need_not_be_contiguous():
    gp = _driver()
    seen, lock = [], threading.Lock()

    def write_one(f, m):
        with lock:
            seen.append((f, int(m[0, 0])))

    with gp.ChunkWriter(2, write_one) as w:
        w.hand_over([0, 1, 2, 17], _images(0, 4))
        w.hand_over([18, 19], _images(4, 2))
    assert sorted(seen) == [(0, 0), (1, 1), (2, 2), (17, 3), (18, 4), (19, 5)]


@pytest.mark.parametrize("bad", [20, 36])
def test_a_writers_exception_reaches_the_caller(bad):
    """Frame 20 is in the second chunk: the third hand-over raises.  Frame 36 is in the last: leaving the block raises."""
    gp = _driver()

    def write_one(f, m):
        if f == bad:
            raise OSError("disk full at frame %d" % f)

    handed = []
    with pytest.raises(OSError, match="disk full at frame %d" % bad):
        with gp.ChunkWriter(3, write_one) as w:
            for first, n in CHUNKS:
                w.hand_over(range(first, first + n), _images(first, n))
                handed.append(first)
    assert handed == ([0, 16] if bad == 20 else [0, 16, 32])


def test_a_chunk_is_submitted_only_after_the_one_before_it_is_done():
    """Chunk k's writes block on an event of the test's.  It is set only once the hand-over of chunk k + 1 has either begun to wait
    or begun to submit, so a hand-over that submitted without waiting would find chunk k pending: at most two chunks are held, the
    one being handed over and the one in flight, and none of chunk k - 2 is pending while chunk k is submitted."""
    gp = _driver()
    gates = [threading.Event() for _ in CHUNKS]
    done, lock, pending_at_submission = set(), threading.Lock(), {}

    def write_one(f, m):
        gates[[k for k, (first, n) in enumerate(CHUNKS) if first <= f < first + n][0]].wait()
        with lock:
            done.add(f)

    def recording(k, reached):
        first, n = CHUNKS[k]
        for i, m in enumerate(_images(first, n)):
            if i == 0:
                with lock:
                    pending_at_submission[k] = sorted(set(range(first)) - done)
                reached.set()
            yield m

    with gp.ChunkWriter(4, write_one) as w:
        wait = w.wait
        for k, (first, n) in enumerate(CHUNKS):
            reached = threading.Event()

            def hooked(reached=reached):
                reached.set()
                wait()
            w.wait = hooked

            def release(k=k, reached=reached):
                reached.wait()
                if k:
                    gates[k - 1].set()
            helper = threading.Thread(target=release)
            helper.start()
            w.hand_over(range(first, first + n), recording(k, reached))
            helper.join()
            assert len(w.held) == n
        w.wait = wait
        gates[-1].set()
    assert pending_at_submission == {0: [], 1: [], 2: []}
    assert done == set(range(37))
