"""The host half of the 16-bit input (hydra_mi.deepio): TiffStack against PIL and against files written here byte by byte,
truncated files, the window and the table against known answers and tests/deep_ref.py, load_video of 16-bit input, and
the two command-line tools resolving the same flags to the same window."""
import argparse
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

import deep_ref as ref

H, W, PAGES = 17, 33, 3


def _pages(dtype=np.uint16, seed=0):
    rng = np.random.default_rng(seed)
    top = 65536 if dtype == np.uint16 else 256
    a = rng.integers(0, top, (PAGES, H, W)).astype(dtype)
    a[0, 0, 0], a[0, 0, 1], a[1, 0, 0] = 0, top - 1, 0x1234 % top
    return a


def _save_pil(path, pages, **kw):
    from PIL import Image
    ims = [Image.fromarray(p) for p in pages]
    ims[0].save(path, format="TIFF", save_all=True, append_images=ims[1:], **kw)
    return path


def _pil_pages(path):
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        return [np.asarray(p).copy() for p in ImageSequence.Iterator(im)]


def _write_tiff(path, pages, bo=">", rows=5, imagej=False):
    """a classic TIFF of 16-bit pages written by hand: `rows` rows per strip, one IFD per page -- or, imagej, the first
    page's IFD alone with images=N in its description and all pages' pixels behind one another"""
    pages = np.asarray(pages)
    n, h, w = pages.shape
    out = bytearray((b"MM" if bo == ">" else b"II") + struct.pack(bo + "HI", 42, 0))
    patch = 4                                                      # where the next IFD's offset goes

    def entry(tag, typ, values):
        data = values if typ == 2 else struct.pack(bo + "%d%s" % (len(values), {3: "H", 4: "I"}[typ]), *values)
        return [tag, typ, len(values), data]
    for k in range(1 if imagej else n):
        data = pages.astype(bo + "u2").tobytes() if imagej else pages[k].astype(bo + "u2").tobytes()
        start = len(out)
        out += data
        strip_rows = h if imagej else rows
        ns = (h + strip_rows - 1) // strip_rows
        offs = [start + i * strip_rows * w * 2 for i in range(ns)]
        counts = [min(strip_rows, h - i * strip_rows) * w * 2 for i in range(ns)]
        es = [entry(256, 3, [w]), entry(257, 3, [h]), entry(258, 3, [16]), entry(259, 3, [1]), entry(262, 3, [1])]
        if imagej:
            es.append(entry(270, 2, b"ImageJ=1.53t\nimages=%d\nslices=%d\n\0" % (n, n)))
        es += [entry(273, 4, offs), entry(277, 3, [1]), entry(278, 3, [strip_rows]), entry(279, 4, counts)]
        if len(out) & 1:
            out += b"\0"
        ifd = len(out)
        out[patch:patch + 4] = struct.pack(bo + "I", ifd)
        extra_at = ifd + 2 + 12 * len(es) + 4
        body, extra = bytearray(struct.pack(bo + "H", len(es))), bytearray()
        for tag, typ, count, d in es:
            if len(d) > 4:
                body += struct.pack(bo + "HHII", tag, typ, count, extra_at + len(extra))
                extra += d + (b"\0" if len(d) & 1 else b"")
            else:
                body += struct.pack(bo + "HHI", tag, typ, count) + d.ljust(4, b"\0")
        patch = ifd + len(body)
        out += body + struct.pack(bo + "I", 0) + extra
    with open(path, "wb") as f:
        f.write(out)
    return path


# ---- TiffStack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["le16", "bigtiff", "u8", "lzw"])
def test_tiffstack_reads_what_pil_reads(hm, tmp_path, kind):
    from hydra_mi import deepio
    pages = _pages(np.uint8 if kind == "u8" else np.uint16)
    kw = {"bigtiff": dict(big_tiff=True), "lzw": dict(compression="tiff_lzw")}.get(kind, {})
    path = _save_pil(str(tmp_path / "s.tif"), pages, **kw)
    if kind == "bigtiff":
        assert open(path, "rb").read(4) in (b"II\x2b\x00", b"MM\x00\x2b")
    want = _pil_pages(path)
    with deepio.TiffStack(path) as st:
        assert len(st) == PAGES and st.shape == (H, W) and st.bits == (8 if kind == "u8" else 16) and st.swap == 0
        assert (st._pil is not None) == (kind == "lzw")           # only the compressed file takes the fallback
        for f in range(PAGES):
            p = st.page(f)
            assert p.shape == (H, W) and np.array_equal(p, want[f]) and np.array_equal(p, pages[f])
        if kind != "lzw":
            assert not st.page(1).flags["OWNDATA"]                # a view of the mapped file


def test_tiffstack_big_endian_strips(hm, tmp_path):
    from hydra_mi import deepio
    pages = _pages()
    path = _write_tiff(str(tmp_path / "be.tif"), pages, ">", rows=5)
    want = _pil_pages(path)                                       # PIL reads the hand-written file too
    with deepio.TiffStack(path) as st:
        assert len(st) == PAGES and st.shape == (H, W) and st.bits == 16 and st.swap == 1
        for f in range(PAGES):
            assert np.array_equal(st.page(f), pages[f]) and np.array_equal(want[f], pages[f])
            assert st.page(f).dtype == np.dtype(">u2")
    path = _write_tiff(str(tmp_path / "le.tif"), pages, "<", rows=5)
    with deepio.TiffStack(path) as st:
        assert st.swap == 0 and all(np.array_equal(st.page(f), pages[f]) for f in range(PAGES))


@pytest.mark.parametrize("bo", ["<", ">"])
def test_tiffstack_imagej_single_ifd(hm, tmp_path, bo):
    from hydra_mi import deepio
    pages = _pages(seed=3)
    path = _write_tiff(str(tmp_path / "ij.tif"), pages, bo, imagej=True)
    with deepio.TiffStack(path) as st:
        assert len(st) == PAGES and st.shape == (H, W) and st.swap == (1 if bo == ">" else 0)
        for f in range(PAGES):
            assert np.array_equal(st.page(f), pages[f])
    data = open(path, "rb").read()
    cut = str(tmp_path / "ij_cut.tif")                            # the IFD is whole, the third page is not
    first = 8
    open(cut, "wb").write(data[:first + 2 * H * W * 2 + 10] + data[first + PAGES * H * W * 2:])
    with pytest.raises(ValueError, match="offset"):
        deepio.TiffStack(cut)


def test_tiffstack_truncated_files(hm, tmp_path):
    """every prefix of a file either reads the pages it holds in full, or raises ValueError and nothing else"""
    from hydra_mi import deepio
    pages = _pages(seed=5)
    data = open(_save_pil(str(tmp_path / "s.tif"), pages), "rb").read()
    path = str(tmp_path / "cut.tif")
    opened = 0
    for n in range(len(data)):
        with open(path, "wb") as f:
            f.write(data[:n])
        try:
            st = deepio.TiffStack(path)
        except ValueError as exc:
            assert "offset" in str(exc), (n, exc)
            continue
        with st:
            opened += 1
            assert st.shape == (H, W) and len(st) <= PAGES
            for k in range(len(st)):
                assert np.array_equal(st.page(k), pages[k]), (n, k)
    assert opened < len(data) // 2
    for junk in (b"", b"II", b"XX*\0\0\0\0\0", b"II*\0\xff\xff\xff\x7f", b"II*\0\x08\0\0\0\xff\xff"):
        with open(path, "wb") as f:
            f.write(junk)
        with pytest.raises(ValueError, match="offset"):
            deepio.TiffStack(path)


# ---- window ----------------------------------------------------------------------------------------------------------
def _hist(d):
    h = np.zeros(65536, np.uint64)
    for v, c in d.items():
        h[v] = c
    return h


def test_window_known_answers(hm):
    from hydra_mi.deepio import window
    assert window(_hist({700: 12345})) == (700, 701)              # a single value: hi <= lo, repaired
    assert window(_hist({0: 5})) == (0, 1)                        # the repair at 0
    assert window(_hist({65535: 5})) == (65534, 65535)            # the repair at 65535
    assert window(_hist({100: 10 ** 6, 4000: 10 ** 6})) == (100, 4000)
    # two values, the upper one rarer than the 10 ppm the default window may clip: hi stays at the lower, repaired
    assert window(_hist({100: 10 ** 6 - 5, 4000: 5})) == (100, 101)
    assert window(_hist({100: 10 ** 6 - 5, 4000: 5}), 1000, 10 ** 6) == (100, 4000)     # hi_ppm = 10^6: the maximum
    h = _hist({10: 1, 20: 998, 30: 1})
    assert window(h, 0, 10 ** 6) == (10, 30)                      # lo_ppm = 0: the minimum
    assert window(h, 1000, 999000) == (20, 21)                    # cum(10) = 1 is not > 1; need = 999 is reached at 20
    assert window(h, 999, 999001) == (10, 30)
    big = _hist({5: 2 ** 62, 9: 2 ** 62})                         # N lo_ppm passes 64 bits
    assert window(big, 500000, 10 ** 6) == (9, 10) and window(big, 499999, 500000) == (5, 6)
    with pytest.raises(ValueError):
        window(np.zeros(65536, np.uint64))
    with pytest.raises(ValueError):
        window(h, -1, 5)


def test_window_equals_the_reference_on_random_histograms(hm):
    from hydra_mi.deepio import window
    rng = np.random.default_rng(11)
    for trial in range(12):
        h = np.zeros(65536, np.uint64)
        k = int(rng.integers(1, 400))
        at = rng.integers(0, 65536, k)
        h[at] = rng.integers(1, 10 ** int(rng.integers(1, 9)), k).astype(np.uint64)
        for lo_ppm, hi_ppm in ((1000, 999990), (0, 10 ** 6), (10 ** 6, 10 ** 6), (0, 0), (int(rng.integers(0, 10 ** 6)), int(rng.integers(0, 10 ** 6)))):
            assert window(h, lo_ppm, hi_ppm) == ref.window(h.tolist(), lo_ppm, hi_ppm), (trial, lo_ppm, hi_ppm)


# ---- make_lut --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 65535), (0, 1), (65534, 65535), (100, 4095), (1000, 1003), (300, 811)])
def test_make_lut_gamma_one(hm, lo, hi):
    from hydra_mi.deepio import make_lut
    lut = make_lut(lo, hi)
    assert lut.dtype == np.uint8 and lut.shape == (65536,)
    assert (np.diff(lut.astype(int)) >= 0).all() and (lut[:lo + 1] == 0).all() and (lut[hi:] == 255).all()
    D = hi - lo
    for v in sorted(set(range(lo, min(hi, lo + 600) + 1)) | set(range(max(lo, hi - 600), hi + 1))):
        x = Fraction(255 * (v - lo), D)
        assert lut[v] == (x + Fraction(1, 2)).__floor__(), v      # round half up
    assert lut.tolist() == ref.make_lut(lo, hi)


def test_make_lut_full_range_and_gamma(hm):
    from hydra_mi.deepio import make_lut
    lut = make_lut(0, 65535)
    assert all(lut[257 * k] == k for k in range(256))
    for gamma in (0.5, 2.2):
        g = make_lut(100, 4095, gamma)
        assert (np.diff(g.astype(int)) >= 0).all() and (g[:101] == 0).all() and (g[4095:] == 255).all()
        assert g.tolist() == ref.make_lut(100, 4095, gamma)
    assert (make_lut(100, 4095, 0.5) >= make_lut(100, 4095)).all()
    for bad in ((5, 5), (6, 5), (-1, 5), (0, 65536)):
        with pytest.raises(ValueError):
            make_lut(*bad)
    with pytest.raises(ValueError):
        make_lut(0, 10, 0.0)


# ---- the host path, load_video ------------------------------------------------------------------------------------------
def _video16(seed=2):
    rng = np.random.default_rng(seed)
    a = rng.integers(900, 1400, (4, H, W)).astype(np.uint16)
    a[2, 3:6, 4:9] = 30000                                        # a bright burst in one frame
    a[1, 0, 0] = 0
    return a


def test_host_path_equals_the_reference(hm):
    from hydra_mi import deepio
    a = _video16()
    h = deepio.histogram(a, device=None)
    assert h.dtype == np.uint64 and h.tolist() == ref.histogram(a.tolist())
    assert np.array_equal(deepio.histogram(a.astype(">u2"), device=None), h)
    lo, hi = deepio.window(h)
    lut = deepio.make_lut(lo, hi)
    frames, clipped = deepio.map_video(a, lut, lo, hi, device=None)
    for f in range(len(a)):
        raw, _, _, clip = ref.map_frame(a[f].reshape(-1).tolist(), lut.tolist(), lo, hi, 0)
        assert frames[f].reshape(-1).tolist() == raw and clipped[f].tolist() == clip
    f2, c2 = deepio.map_video(a.astype(">u2"), lut, lo, hi, device=None)
    assert np.array_equal(f2, frames) and np.array_equal(c2, clipped)


def test_load_video_takes_16_bit_input(hm, tmp_path):
    from hydra_mi import deepio, pipeline
    a = _video16()
    npy, tif = str(tmp_path / "v.npy"), _save_pil(str(tmp_path / "v.tif"), a)
    np.save(npy, a)
    be = _write_tiff(str(tmp_path / "be.tif"), a, ">", rows=5)
    h = np.bincount(a.reshape(-1), minlength=65536)
    lo, hi = deepio.window(h)
    assert (lo, hi) == ref.window(h.tolist())                     # the default window over every frame
    for fn in (npy, tif, be):
        got = pipeline.load_video(fn)
        assert got.dtype == np.uint8 and np.array_equal(got, deepio.make_lut(lo, hi)[a])
        got = pipeline.load_video(fn, depth=dict(lo=950, hi=30000, gamma=0.5))
        assert np.array_equal(got, deepio.make_lut(950, 30000, 0.5)[a])
        got = pipeline.load_video(fn, depth=dict(lo_ppm=0, hi_ppm=10 ** 6))
        assert np.array_equal(got, deepio.make_lut(0, 30000)[a])
    with pytest.raises(ValueError):
        pipeline.load_video(npy, depth=dict(lo=5))
    with pytest.raises(ValueError):
        pipeline.load_video(npy, depth=dict(lo=7, hi=7))


def test_load_video_of_8_bit_input_is_unchanged(hm, tmp_path):
    from hydra_mi import pipeline
    a = _pages(np.uint8)
    npy, tif = str(tmp_path / "v.npy"), _save_pil(str(tmp_path / "v.tif"), a)
    np.save(npy, a)
    for fn in (npy, tif):
        assert np.array_equal(pipeline.load_video(fn), a)
        assert np.array_equal(pipeline.load_video(fn, depth=dict(lo=1, hi=2)), a)     # depth does nothing to 8-bit input
    bgr = np.random.default_rng(0).integers(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    np.save(npy, bgr)
    assert np.array_equal(pipeline.load_video(npy), pipeline.to_gray(bgr))
    np.save(npy, a.astype(np.float32))
    with pytest.raises(ValueError, match="8-bit"):
        pipeline.load_video(npy)


def test_open_deep_peeks_at_archives(hm, tmp_path, monkeypatch):
    """an .npz is recognised by its first member's header: 16-bit frames are loaded, an 8-bit archive is left unread"""
    from hydra_mi import deepio, pipeline
    a16, a8 = _video16(), _pages(np.uint8)
    p16, p8, pc = str(tmp_path / "d.npz"), str(tmp_path / "e.npz"), str(tmp_path / "c.npz")
    np.savez(p16, video=a16)
    np.savez(p8, video=a8)
    np.savez_compressed(pc, video=a16)
    for p in (p16, pc):
        got = deepio.open_deep(p)
        assert isinstance(got, np.ndarray) and np.array_equal(got, a16)
    assert np.array_equal(pipeline.load_video(pc, depth=dict(lo=950, hi=30000)), deepio.make_lut(950, 30000)[a16])
    reads = []
    real = np.lib.npyio.NpzFile.__getitem__
    monkeypatch.setattr(np.lib.npyio.NpzFile, "__getitem__", lambda self, key: (reads.append(key), real(self, key))[1])
    assert deepio.open_deep(p8) is None and reads == []           # the header alone was read
    assert np.array_equal(pipeline.load_video(p8), a8) and reads == ["video"]
    assert deepio.open_deep(str(tmp_path / "missing.npy")) is None
    with pytest.raises(ValueError, match="threshold 300 outside 0..255"):
        deepio.DeepSource(a16, deepio.make_lut(1, 2), 1, 2, 300)


# ---- the command-line tools --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["--depth-range", "950,30000"], ["--depth-percentiles", "0,1000000", "--depth-gamma", "0.5"],
                                   ["--depth-gamma", "2"]])
def test_both_tools_resolve_the_flags_to_one_window(hm, flags):
    from hydra_mi import deepio
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import optical_flow_ext as flow_cli
    import run_kalmanfilter as track_cli
    parser = argparse.ArgumentParser()
    track_cli.add_depth_arguments(parser)
    d_track = track_cli.depth_of(parser.parse_args(flags))
    rest, d_flow = flow_cli._depth_opts(["prog"] + flags + ["v.npy", "out"])
    assert rest == ["prog", "v.npy", "out"] and d_track == d_flow
    if not flags:
        assert d_track is None
    a = _video16()
    wa, wb = deepio.resolve(a, d_track, device=None), deepio.resolve(a, d_flow, device=None)
    assert (wa["lo"], wa["hi"], wa["gamma"]) == (wb["lo"], wb["hi"], wb["gamma"]) and np.array_equal(wa["lut"], wb["lut"])
    if flags[:1] == ["--depth-range"]:
        assert (wa["lo"], wa["hi"]) == (950, 30000)
    for bad in (["--depth-range", "5"], ["--depth-range", "1,2", "--depth-percentiles", "1,2"], ["--depth-gamma", "-1"]):
        with pytest.raises(ValueError):
            track_cli.depth_of(parser.parse_args(bad))
        with pytest.raises(ValueError):
            flow_cli._depth_opts(bad)


def test_clip_warning_is_a_condition(hm):
    from hydra_mi.deepio import clip_warning
    clipped = np.array([[0, 1], [3, 100], [0, 101]], np.uint32)
    assert clip_warning(np.array([[0, 100]]), 10 ** 6) is None            # 100 ppm = 10 x 10 ppm: not more
    line = clip_warning(clipped, 10 ** 6)
    assert line is not None and "frame 2" in line and "0.0101 %" in line
