"""CPU checks of the tracker's output files: the library's AVI container read back by a RIFF parser of its own (headers,
frame count, row padding, the OpenDML continuation through indx / ix00), PNG round trips, and the command-line tools
writing nothing new unless asked (-n, an .avi fn_out, HYDRA_MI_FLOW_PREVIEW=1)."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a small RIFF / AVI reader ---------------------------------------------------------------------------------------
def _chunks(b, start, end):
    """(fourcc, data offset, size[, list type]) of the chunks in b[start:end]"""
    out = []
    p = start
    while p + 8 <= end:
        cc, size = b[p:p + 4].decode("latin-1"), struct.unpack_from("<I", b, p + 4)[0]
        if cc in ("RIFF", "LIST"):
            out.append((cc, p + 12, size - 4, b[p + 8:p + 12].decode("latin-1")))
        else:
            out.append((cc, p + 8, size, None))
        p += 8 + size + (size & 1)
    return out


def read_avi(path):
    b = open(path, "rb").read()
    riffs = _chunks(b, 0, len(b))
    assert riffs and riffs[0][0] == "RIFF" and riffs[0][3] == "AVI "
    assert all(r[0] == "RIFF" and r[3] == "AVIX" for r in riffs[1:])
    assert sum(8 + 4 + r[2] for r in riffs) == len(b)             # the RIFF sizes add up to the file
    top = {c[3] or c[0]: c for c in _chunks(b, riffs[0][1], riffs[0][1] + riffs[0][2])}
    hdrl = {c[3] or c[0]: c for c in _chunks(b, top["hdrl"][1], top["hdrl"][1] + top["hdrl"][2])}
    avih = struct.unpack_from("<10I", b, hdrl["avih"][1])
    strl = {c[3] or c[0]: c for c in _chunks(b, hdrl["strl"][1], hdrl["strl"][1] + hdrl["strl"][2])}
    strh = b[strl["strh"][1]:strl["strh"][1] + 56]
    bih = struct.unpack_from("<IiiHHIIiiII", b, strl["strf"][1])
    odml = _chunks(b, hdrl["odml"][1], hdrl["odml"][1] + hdrl["odml"][2])
    dmlh_total = struct.unpack_from("<I", b, odml[0][1])[0]
    info = dict(us_per_frame=avih[0], avih_frames=avih[4], streams=avih[6], width=avih[8], height=avih[9],
                fcc_type=strh[0:4], handler=strh[4:8], scale=struct.unpack_from("<I", strh, 20)[0],
                rate=struct.unpack_from("<I", strh, 24)[0], length=struct.unpack_from("<I", strh, 32)[0],
                bih=bih, total=dmlh_total, riffs=len(riffs))
    W, H = bih[1], bih[2]
    stride = (3 * W + 3) & ~3
    assert bih[0] == 40 and bih[4] == 24 and bih[5] == 0 and bih[6] == stride * H and H > 0   # BI_RGB, bottom-up

    def frame_at(off):
        rows = np.frombuffer(b, np.uint8, stride * H, off).reshape(H, stride)
        assert not rows[:, 3 * W:].any()                            # the padding is zero
        return rows[::-1, :3 * W].reshape(H, W, 3)

    # legacy index of the first RIFF
    movi0 = top["movi"]
    idx1 = top["idx1"]
    n1 = idx1[2] // 16
    legacy = []
    for i in range(n1):
        ck, flags, off, size = struct.unpack_from("<4sIII", b, idx1[1] + 16 * i)
        assert ck == b"00db" and flags & 0x10 and size == stride * H
        p = movi0[1] - 4 + off                                     # relative to the 'movi' fourcc
        assert b[p:p + 4] == b"00db"
        legacy.append(frame_at(p + 8))
    # OpenDML: super index -> ix00 -> frames
    indx = strl["indx"]
    wl, sub, typ, used, cid = struct.unpack_from("<HBBI4s", b, indx[1])
    assert (wl, sub, typ, cid) == (4, 0, 0, b"00db")
    frames = []
    for e in range(used):
        off, size, dur = struct.unpack_from("<QII", b, indx[1] + 24 + 16 * e)
        assert b[off:off + 4] == b"ix00" and struct.unpack_from("<I", b, off + 4)[0] + 8 == size
        wl2, sub2, typ2, n, cid2, base = struct.unpack_from("<HBBI4sQ", b, off + 8)
        assert (wl2, sub2, typ2, cid2) == (2, 0, 1, b"00db") and n == dur
        for i in range(n):
            o, s = struct.unpack_from("<II", b, off + 32 + 8 * i)
            assert s == stride * H and b[base + o - 8:base + o - 4] == b"00db"
            frames.append(frame_at(base + o))
    info["frames"], info["legacy"], info["idx1_frames"] = frames, legacy, n1
    return info


def _frames(n, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def test_avi_headers_count_and_padding(hm, tmp_path):
    from hydra_mi.videoio import AviWriter
    H, W, n = 72, 90, 5                                             # 270 bytes a row: 2 bytes of padding
    fr = _frames(n, H, W)
    path = str(tmp_path / "v.avi")
    with AviWriter(path, W, H) as v:
        for f in fr:
            v.write(f)
    info = read_avi(path)
    assert info["us_per_frame"] == 50000 and info["rate"] == 20 and info["scale"] == 1       # 20 frames/s
    assert (info["width"], info["height"]) == (W, H) and info["streams"] == 1
    assert info["fcc_type"] == b"vids" and info["handler"] == b"DIB "
    assert info["avih_frames"] == n and info["length"] == n and info["total"] == n and info["riffs"] == 1
    assert info["idx1_frames"] == n
    assert all(np.array_equal(a, b) for a, b in zip(info["frames"], fr)) and len(info["frames"]) == n
    assert all(np.array_equal(a, b) for a, b in zip(info["legacy"], fr))


def test_avi_opendml_continuation(hm, tmp_path):
    from hydra_mi.videoio import AviWriter
    H, W, n = 33, 45, 23                                            # odd sizes: 135 bytes a row, 1 of padding
    fr = _frames(n, H, W, 1)
    path = str(tmp_path / "long.avi")
    limit = 160 * 1024                                               # 23 frames of 4.5 KB: one RIFF
    with AviWriter(path, W, H, riff_limit=limit) as v:
        for f in fr:
            v.write(f)
    info = read_avi(path)
    assert info["riffs"] == 1 and len(info["frames"]) == n
    # several RIFFs: the headers and three frames per RIFF
    path2 = str(tmp_path / "long2.avi")
    stride = (3 * W + 3) & ~3
    with AviWriter(path2, W, H, riff_limit=16384 + 3 * stride * H) as v:
        for f in fr:
            v.write(f)
    info = read_avi(path2)
    assert info["riffs"] >= 3, info["riffs"]
    assert info["total"] == n and info["length"] == n
    assert info["avih_frames"] == info["idx1_frames"] < n           # the first RIFF's own count
    assert len(info["frames"]) == n
    assert all(np.array_equal(a, b) for a, b in zip(info["frames"], fr))
    assert all(np.array_equal(a, b) for a, b in zip(info["legacy"], fr[:info["idx1_frames"]]))


def test_avi_argument_errors(hm, tmp_path):
    from hydra_mi.videoio import AviWriter
    with pytest.raises(RuntimeError, match="frame size"):
        AviWriter(str(tmp_path / "x.avi"), 0, 10)
    with pytest.raises(RuntimeError, match="RIFF limit"):
        AviWriter(str(tmp_path / "x.avi"), 64, 64, riff_limit=1000)
    with pytest.raises(RuntimeError, match="cannot open"):
        AviWriter(str(tmp_path / "no" / "x.avi"), 8, 8)
    with AviWriter(str(tmp_path / "y.avi"), 8, 8) as v:
        with pytest.raises(ValueError):
            v.write(np.zeros((8, 9, 3), np.uint8))


def test_png_round_trip(hm, tmp_path):
    from hydra_mi.videoio import read_png, write_png
    img = _frames(1, 37, 53, 2)[0]
    p = write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(read_png(p), img)
    from PIL import Image
    rgb = np.asarray(Image.open(p))
    assert np.array_equal(rgb[:, :, 0], img[:, :, 2])             # B G R in memory, R G B in the file


# ---- the command-line tools with stubs: nothing new is written unless asked --------------------------------------------
class _StubKF:
    def __init__(self, distmesh, frame, flow, cuda=True, **kw):
        self.state = type("S", (), {})()
        self.state.X = np.zeros((8, 1))
        self.state.tri = np.zeros((1, 3), np.int32)
        self.shots = []

    def compute(self, *a, **kw):
        assert kw.get("imageoutput") is None
        return (0, 0.0, 0.0, 0, None, None)

    def screenshots(self, basename):
        self.shots.append(basename)


class _StubVideo:
    def __init__(self, fn, threshold):
        self.k = 0

    def current_frame(self):
        return np.zeros((8, 8), np.uint8)

    def backsub(self):
        return np.zeros((8, 8), np.uint8), None, None

    def isOpened(self):
        return self.k < 3

    def read(self):
        self.k += 1
        z = np.zeros((8, 8), np.uint8)
        return (self.k < 3), z, z, z


class _StubMesh:
    def __init__(self, frame, h0):
        self.p = np.zeros((4, 2))

    def createMesh(self, *a, **kw):
        pass


class _StubFlow:
    def __init__(self, path):
        pass

    def peek(self):
        return True, np.zeros((8, 8, 2), np.float32)

    read = peek


def _cli(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import run_kalmanfilter as cli
    monkeypatch.setattr(cli, "VideoStream", _StubVideo)
    monkeypatch.setattr(cli, "DistMesh", _StubMesh)
    monkeypatch.setattr(cli, "FlowStream", _StubFlow)
    monkeypatch.setattr(cli.kalman, "IteratedMSKalmanFilter", _StubKF)
    monkeypatch.chdir(tmp_path)
    return cli


def test_cli_writes_only_the_states_without_n_or_avi(hm, monkeypatch, tmp_path):
    cli = _cli(monkeypatch, tmp_path)
    made = []
    monkeypatch.setattr(cli, "AviWriter", lambda *a, **k: made.append(a))
    assert cli.main(["in.npy", "flow", "out.npz"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["out.npz"]
    assert made == []


def test_cli_n_and_avi_are_recognised(hm, monkeypatch, tmp_path):
    cli = _cli(monkeypatch, tmp_path)
    opened = []

    class _W:
        def __init__(self, path, W, H):
            opened.append((path, W, H))
            self.frames = 0

        def write(self, img):
            self.frames += 1

        def close(self):
            pass

    monkeypatch.setattr(cli, "AviWriter", _W)
    kfs = []
    orig = _StubKF.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        kfs.append(self)
    monkeypatch.setattr(_StubKF, "__init__", init)
    monkeypatch.setattr(_StubKF, "state", None, raising=False)

    class _R:
        def view(self, X, which):
            assert which == "overlay"
            return np.zeros((8, 8, 3), np.uint8)

    def compute(self, *a, **kw):
        self.state.renderer = _R()
        return (0, 0.0, 0.0, 0, None, None)
    monkeypatch.setattr(_StubKF, "compute", compute)
    assert cli.main(["in.npy", "flow", "out.avi", "-n", "run"]) == 0
    assert opened == [("out.avi", 8, 8)]
    assert os.path.exists("out.avi.npz") and os.path.isdir("screenshots")
    assert kfs[0].shots == ["screenshots/run_frame_1", "screenshots/run_frame_2"]


def test_flow_tool_writes_no_preview_without_the_variable(hm, monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import optical_flow_ext as tool
    from hydra_mi import videoio

    class _BF:
        def __init__(self, *a, **k):
            pass

        def calc_batch(self, f0, f1):
            return np.zeros(f0.shape, np.float32), np.zeros(f0.shape, np.float32)

    monkeypatch.setattr(tool.brox, "BroxOpticalFlow", _BF)
    np.save(str(tmp_path / "v.npy"), np.zeros((3, 6, 7), np.uint8))
    monkeypatch.chdir(tmp_path)
    made = []
    monkeypatch.setattr(videoio, "AviWriter", lambda *a, **k: made.append(a))
    monkeypatch.delenv("HYDRA_MI_FLOW_PREVIEW", raising=False)
    assert tool.main(["x", "v.npy", "f"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["f_000_x.mat", "f_000_y.mat", "f_001_x.mat", "f_001_y.mat", "v.npy"]
    assert made == []
