"""The JPEG files both Motion-JPEG decoder tests use (test_mjpeg_dec_cpu.py, test_mjpeg_dec_gpu.py): files of the encoder's
restatement (mjpeg_ref) and of PIL, the malformed streams, and small AVI containers assembled from the AVI rules."""
import io
import struct

import numpy as np

import mjpeg_dec_ref
import mjpeg_ref

SIZES = ((1, 1), (7, 9), (8, 8), (9, 8), (17, 17), (61, 45))      # W x H; 17 x 17: a second, mostly padded MCU at 4:2:0
FORMS = (("plain", {}), ("rows1", {"restart_marker_rows": 1}), ("blocks3", {"restart_marker_blocks": 3}),
         ("optimize", {"optimize": True}))
#: cases of mjpeg_ref.cases() that stress the decoder's structure (the GPU test runs these beside the small ones)
STRUCTURAL = ("wide_2056x8_c1", "turns_8200x8_c1", "tall_8x2056_c1", "restart_24x80_r1", "restart_24x80_r3", "dc11", "ac10",
              "noise_q100")


def image(W, H, channels):
    f = mjpeg_ref.smooth_image(W, H, channels).astype(np.int16)
    noise = np.random.default_rng(W * 100 + H + channels).integers(-20, 21, f.shape)
    return np.clip(f + noise, 0, 255).astype(np.uint8)


def pil_save(a, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])).save(b, "JPEG", **kw)
    return b.getvalue()


def pil_grey(data):
    """libjpeg's own grey output of a file: the component of a grey file, the luma plane of a colour one"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode != "L":
        im.draft("L", im.size)
    assert im.mode == "L", im.mode
    return np.asarray(im).copy()


def segments(data):
    """[(marker, offset of the FF, length with the marker)] up to and including SOS"""
    out, p = [], 2
    while True:
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.append((m, p, n + 2))
        p += n + 2
        if m == 0xDA:
            return out


def without(data, marker):
    for m, p, n in reversed(segments(data)):
        if m == marker:
            data = data[:p] + data[p + n:]
    return data


def small_files():
    """[(key, file bytes)]: every small case; the expectation of each is mjpeg_dec_ref.reference(key, data)"""
    out = []
    for name, frame, q, rr in mjpeg_ref.cases():
        if frame.shape[0] * frame.shape[1] <= 61 * 45:
            out.append(("enc_" + name, mjpeg_ref.reference(name)[0]))
    for W, H in SIZES:
        for sub in (0, 1, 2):
            for form, kw in FORMS:
                out.append(("pil_%dx%d_s%d_%s" % (W, H, sub, form), pil_save(image(W, H, 3), quality=90, subsampling=sub, **kw)))
    for q in (5, 50, 90, 100):
        for form, kw in FORMS[:3]:
            out.append(("pil_grey_q%d_%s" % (q, form), pil_save(image(61, 45, 1), quality=q, **kw)))
        out.append(("pil_420_q%d" % q, pil_save(image(61, 45, 3), quality=q, subsampling=2)))
    plain = pil_save(image(61, 45, 3), quality=75, subsampling=1, restart_marker_rows=1)
    out.append(("no_dht", without(plain, 0xC4)))
    sos = [s for s in segments(plain) if s[0] == 0xDA][0][1]
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body      # noqa: E731
    out.append(("com_app_fill", plain[:2] + seg(0xFE, b"a comment") + plain[2:sos] + seg(0xE5, b"\x01\x02\x03") + b"\xff\xff\xff"
                + plain[sos:]))
    return out


def large_files():
    return [("enc_" + name, mjpeg_ref.reference(name)[0]) for name, frame, q, rr in mjpeg_ref.cases()
            if frame.shape[0] * frame.shape[1] > 61 * 45]


def structural_files():
    return [("enc_" + name, mjpeg_ref.reference(name)[0]) for name in STRUCTURAL]


# ---- malformed streams ----------------------------------------------------------------------------------------------
def _stuffed(bits):
    b = mjpeg_ref._Bits()
    for ch in bits:
        b.bits.append(int(ch))
    return b.stuffed()


def _code(table, symbol):
    code, length = table[symbol]
    return format(code, "0%db" % length)


def with_interval(data, idx, new):
    start, end, _ = mjpeg_dec_ref.parse(data)["intervals"][idx]
    return data[:start] + new + data[end:]


def malformed():
    """-> (clean file, [(name, file)]): a grey 32 x 32 frame of four intervals of four blocks whose interval 1 is damaged"""
    clean = mjpeg_ref.encode(np.random.default_rng(11).integers(0, 256, (32, 32), dtype=np.uint8), 75, 1)[0]
    start, end, _ = mjpeg_dec_ref.parse(clean)["intervals"][1]
    dc = mjpeg_ref.huffman(mjpeg_ref.DC_BITS[0], mjpeg_ref.DC_VALS)
    ac = mjpeg_ref.huffman(mjpeg_ref.AC_BITS[0], mjpeg_ref.AC_VALS[0])
    out = [("truncated", with_interval(clean, 1, clean[start:start + (end - start) // 2])),
           ("undefined_code", with_interval(clean, 1, _stuffed("1" * 48))),
           ("run_past_63", with_interval(clean, 1, _stuffed(_code(dc, 0) + _code(ac, 0xF0) * 4)))]
    # a DC table whose longest code means category 12
    dht = [s for s in segments(clean) if s[0] == 0xC4 and clean[s[1] + 4] == 0x00][0]
    at = dht[1] + 5 + 16 + 11
    assert clean[at] == 11
    twelve = clean[:at] + b"\x0c" + clean[at + 1:]
    out.append(("dc_size_12", with_interval(twelve, 1, _stuffed(_code(dc, 11) + "1" * 12))))
    return clean, out


# ---- AVI containers, from the AVI rules -----------------------------------------------------------------------------
def chunk(cc, body):
    return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def lst(kind, form, parts):
    return chunk(kind, form + b"".join(parts))[:]


def strl(kind, handler, strf, scale=1, rate=20):
    strh = kind + handler + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0, 0)
    return lst(b"LIST", b"strl", [chunk(b"strh", strh), chunk(b"strf", strf)])


def bitmapinfo(W, H, bits, compression):
    comp = compression if isinstance(compression, int) else struct.unpack("<I", compression)[0]
    return struct.pack("<IiiHHIIiiII", 40, W, H, 1, bits, comp, 0, 0, 0, 0, 0)


def raw_rows(bgr, top_down):
    H, W = bgr.shape[:2]
    stride = (3 * W + 3) & ~3
    rows = np.zeros((H, stride), np.uint8)
    rows[:, :3 * W] = bgr.reshape(H, 3 * W)
    return (rows if top_down else rows[::-1]).tobytes()


def foreign_avi(frames):
    """Four B G R frames -> (file bytes, the frames a reader must give): audio as stream 0, the video as stream 1 and
    top-down, JUNK, a 'rec ' list, odd chunk sizes, a dropped frame (frame 2 repeats frame 1), 'idx1' and an 'AVIX' RIFF."""
    H, W = frames[0].shape[:2]
    avih = struct.pack("<14I", 50000, 0, 0, 0x10, 4, 0, 2, 0, W, H, 0, 0, 0, 0)
    audio = strl(b"auds", b"\0\0\0\0", struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8), 1, 8000)
    video = strl(b"vids", b"DIB ", bitmapinfo(W, -H, 24, 0), 1, 25)
    hdrl = lst(b"LIST", b"hdrl", [chunk(b"avih", avih), audio, video, chunk(b"JUNK", b"\0" * 7)])
    v = [chunk(b"01db", raw_rows(f, True)) for f in frames]
    movi = lst(b"LIST", b"movi", [chunk(b"00wb", b"\x80" * 13), v[0], chunk(b"ix01", b"\0" * 9),
                                  lst(b"LIST", b"rec ", [v[1], chunk(b"00wb", b"\x80" * 5)]), chunk(b"01db", b""),
                                  chunk(b"JUNK", b"\0" * 3)])
    first = lst(b"RIFF", b"AVI ", [hdrl, chunk(b"JUNK", b"\0" * 11), movi, chunk(b"idx1", b"\0" * 32)])
    second = lst(b"RIFF", b"AVIX", [lst(b"LIST", b"movi", [v[3]])])
    return first + second, [frames[0], frames[1], frames[1], frames[3]]


def tiny_avi(strf):
    """a one-stream AVI with the given stream format and no frames"""
    avih = struct.pack("<14I", 50000, 0, 0, 0x10, 0, 0, 1, 0, 8, 8, 0, 0, 0, 0)
    hdrl = lst(b"LIST", b"hdrl", [chunk(b"avih", avih), strl(b"vids", b"\0\0\0\0", strf)])
    return lst(b"RIFF", b"AVI ", [hdrl, lst(b"LIST", b"movi", [])])
