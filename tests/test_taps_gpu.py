"""The writer-thread error path the two taps share (`pytest -m gpu`): an exception the writer thread meets (here: the
AviWriter refuses its second frame) is stored, the slots queued behind it are skipped and given back, and the exception
is reported by drain(), by every later frame() / push() -- which queue nothing -- and once by close().  Nothing is done
to the device: the exception is a Python one, raised on the writer thread."""
import threading

import numpy as np
import pytest

from test_body_gpu import _filter, _scene

pytestmark = pytest.mark.gpu


def _failing(base, method):
    """An AviWriter whose `method` (write_ptr, write_chunk_ptr) raises OSError on its second call -- once `gate` is set,
    so that the test decides how many frames are queued before the writer thread fails."""
    class Failing(base):
        calls = 0
        gate = None

        def _fail_second(self, *args):
            self.calls += 1
            if self.calls == 2:
                self.gate.wait(60)
                raise OSError("injected: the disk is full")
            return getattr(base, method)(self, *args)
    setattr(Failing, method, Failing._fail_second)
    return Failing


def _writer(path, W, H, method, **opts):
    from hydra_mi.videoio import AviWriter
    w = _failing(AviWriter, method)(str(path), W, H, **opts)
    w.gate = threading.Event()
    return w


def _scene16():
    dm, Xs, frames, f0 = _scene("16")
    kf = _filter(dm, f0)
    H, W = f0.shape                                         # (the overlay shows the observed frame)
    kf.state.renderer.set_observation(f0, np.zeros((H, W, 2), np.float32), (f0 > 0).astype(np.uint8))
    return kf, Xs, frames


def _push_five(push, writer):
    """Five frames over two slots: the third reuses the slot of the first and is queued before the writer fails (the
    gate); the failure may then reach the fourth or fifth frame() already -- that is its report, and nothing more is
    pushed.  -> frames queued"""
    queued = 0
    for k in range(5):
        try:
            push(k)
        except OSError as e:
            assert k >= 3 and "injected" in str(e)
            break
        queued += 1
        if k == 2:
            writer.gate.set()
    assert queued >= 3
    return queued


def _check_reports(tap, writer, push_more, queued_by_push_more):
    with pytest.raises(OSError, match="injected") as first:
        tap.drain()                                         # returns: every slot was given back
    before = queued_by_push_more()
    with pytest.raises(OSError, match="injected") as again:
        push_more()
    assert again.value is first.value
    assert queued_by_push_more() == before                  # the refused frame queued nothing
    with pytest.raises(OSError, match="injected") as closing:
        tap.close()
    assert closing.value is first.value
    tap.close()                                             # the second close() returns
    assert writer.frames == 1 and writer.calls >= 2
    assert not tap._thread.is_alive()


@pytest.mark.parametrize("codec", ["raw", "mjpeg"])
def test_video_tap_reports_the_writers_error(hm, tmp_path, codec):
    from hydra_mi.pipeline import VideoTap
    kf, Xs, _ = _scene16()
    r = kf.state.renderer
    opts = dict(codec="mjpeg", quality=90) if codec == "mjpeg" else {}
    w = _writer(tmp_path / "v.avi", r.nx, r.ny, "write_chunk_ptr" if codec == "mjpeg" else "write_ptr", **opts)
    tap = VideoTap(r, w, slots=2)
    assert tap._thread.name == "hydra_mi-video"
    _push_five(lambda k: tap.frame(Xs[k % len(Xs)]), w)
    views = []

    def queue_view(d_out, stream):
        views.append(d_out)
        r.view_dev(Xs[0], "overlay", d_out, stream)
    _check_reports(tap, w, lambda: tap.push(queue_view), lambda: len(views))
    with pytest.raises(OSError, match="injected"):
        tap.frame(Xs[0])
    w.close()
    kf.close()


def test_body_tap_reports_the_writers_error(hm, tmp_path):
    from hydra_mi import body
    from hydra_mi.pipeline import DeviceBuffer
    kf, Xs, frames = _scene16()
    r = kf.state.renderer
    w = _writer(tmp_path / "reg.avi", r.nx, r.ny, "write_ptr")
    b = body.BodyReadout(kf, points=np.array([[7.5, 7.5]]), video=w)
    tap = body.BodyTap(b, slots=2)
    assert tap._thread.name == "hydra_mi-body"
    d_frame = DeviceBuffer(r.nx * r.ny)
    d_frame.upload(frames[0])
    queued = _push_five(lambda k: tap.frame(Xs[k % len(Xs)], d_frame.ptr), w)
    assert len(b._rows) == queued
    _check_reports(tap, w, lambda: tap.frame(Xs[0], d_frame.ptr), lambda: len(b._rows))
    # the frame written before the failure brought its sums; the frames skipped behind it brought none
    assert b._rows[0][1] is not None and np.array_equal(b._rows[0][1], r.body_warp(Xs[0], frames[0])[1])
    assert all(row[1] is None for row in b._rows[2:])
    d_frame.close()
    w.close()
    kf.close()
