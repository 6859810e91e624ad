"""The Motion-JPEG encoder of include/hydra_mi.h restated in loops and Python integers, from the rules written there and
not from the kernel: ``encode`` gives a frame's whole JPEG file and a histogram of the symbols it emitted.  The device
must give these bytes.  Slow on purpose (a 61x45 colour frame takes a fraction of a second)."""
import math

import numpy as np

# ITU-T T.81 Annex K, tables K.1 and K.2 (natural order)
QUANT = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
     62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
     112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
     99) + (99,) * 32,
)
# tables K.3 - K.6: (BITS, HUFFVAL) of DC 0, DC 1, AC 0, AC 1
DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
DC_VALS = tuple(range(12))
AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77))
AC_VALS = (
    bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
                  "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
                  "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
                  "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
                  "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)
ROW_SHIFT, COL_SHIFT = 11, 12            # 13 - 2: two fractional bits between the passes; 13 + 2 - 3: three in the result
COEF_ONE = 8                             # a coefficient is held in eighths


def zigzag():
    """natural index of every zigzag position, walked along the anti-diagonals"""
    order = []
    for d in range(15):
        rows = [r for r in range(8) if 0 <= d - r < 8]                     # odd diagonals run down-left: rows ascending
        if d % 2 == 0:
            rows.reverse()                                                 # even diagonals run up-right
        order += [8 * r + (d - r) for r in rows]
    return order


ZIGZAG = zigzag()


def dct_table():
    return [[int(round(8192 * ((1 / math.sqrt(2)) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)))
             for x in range(8)] for u in range(8)]


T = dct_table()


def dct_bound():
    """E with |fixed / 8 - exact| <= E for every coefficient of a block of samples in -128..127."""
    exact = [[8192 * ((1 / math.sqrt(2)) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
             for u in range(8)]
    dt = max(sum(abs(T[u][x] - exact[u][x]) for x in range(8)) for u in range(8))      # a row's table error
    at = max(sum(abs(exact[u][x]) for x in range(8)) for u in range(8))                # a row's exact weight
    e_row = dt * 128 / 2 ** ROW_SHIFT + 0.5                                            # |r - r*|
    r_max = 128 * max(sum(abs(T[u][x]) for x in range(8)) for u in range(8)) / 2 ** ROW_SHIFT + 0.5
    return ((at * e_row + dt * r_max) / 2 ** COL_SHIFT + 0.5) / COEF_ONE


def fdct(block):
    """block[y][x] in -128..127 -> c8[v][u], eight times the coefficient, v the vertical frequency"""
    r = [[(sum(T[u][x] * block[y][x] for x in range(8)) + (1 << (ROW_SHIFT - 1))) >> ROW_SHIFT for u in range(8)]
         for y in range(8)]
    return [[(sum(T[v][y] * r[y][u] for y in range(8)) + (1 << (COL_SHIFT - 1))) >> COL_SHIFT for u in range(8)]
            for v in range(8)]


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(255, max(1, (v * s + 50) // 100)) for v in tab] for tab in QUANT]


def huffman(bits, vals):
    """symbol -> (code, length), the canonical codes of T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(W, H, channels, quality, restart_rows=1):
    q = quant_tables(quality)
    sets = 2 if channels == 3 else 1
    bw, bh = (W + 7) // 8, (H + 7) // 8
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for s in range(sets):
        out += _seg(0xDB, bytes([s] + [q[s][ZIGZAG[k]] for k in range(64)]))
    sof = [8] + list(H.to_bytes(2, "big")) + list(W.to_bytes(2, "big")) + [channels]
    for c in range(channels):
        sof += [c + 1, 0x11, 1 if c else 0]
    out += _seg(0xC0, sof)
    for s in range(sets):
        out += _seg(0xC4, bytes([s]) + bytes(DC_BITS[s]) + bytes(DC_VALS))
        out += _seg(0xC4, bytes([0x10 | s]) + bytes(AC_BITS[s]) + bytes(AC_VALS[s]))
    out += _seg(0xDD, (bw * min(restart_rows, bh)).to_bytes(2, "big"))
    sos = [channels]
    for c in range(channels):
        sos += [c + 1, 0x11 if c else 0x00]
    return out + _seg(0xDA, sos + [0, 63, 0])


def _samples(frame, channels):
    """-> per component an H x W list of lists of samples less 128"""
    a = np.asarray(frame, np.uint8)
    H, W = a.shape[:2]
    if channels == 1:
        return [[[int(a[y, x]) - 128 for x in range(W)] for y in range(H)]]
    planes = [[], [], []]
    for y in range(H):
        rows = [[], [], []]
        for x in range(W):
            B, G, R = int(a[y, x, 0]), int(a[y, x, 1]), int(a[y, x, 2])
            rows[0].append(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128)
            rows[1].append(((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128)
            rows[2].append(((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128)
        for c in range(3):
            planes[c].append(rows[c])
    return planes


def _category(v):
    return abs(v).bit_length()


class _Bits:
    def __init__(self):
        self.bits = []

    def put(self, code, length):
        for i in range(length - 1, -1, -1):
            self.bits.append((code >> i) & 1)

    def value(self, v, size):
        self.put((v - 1 if v < 0 else v) & ((1 << size) - 1), size)

    def stuffed(self):
        while len(self.bits) % 8:
            self.bits.append(1)
        out = bytearray()
        for i in range(0, len(self.bits), 8):
            b = 0
            for bit in self.bits[i:i + 8]:
                b = (b << 1) | bit
            out.append(b)
            if b == 0xFF:
                out.append(0)
        return bytes(out)


def encode(frame, quality=90, restart_rows=1, channels=None):
    """frame (H, W) or (H, W, 3) B G R uint8 -> (the JPEG file's bytes, histogram).  The histogram counts "dc<category>",
    "ac<size>", "zrl", "eob", "no_eob" (blocks that end in a non-zero coefficient), "stuffed" (FF 00 pairs) and
    "intervals"."""
    a = np.asarray(frame, np.uint8)
    if channels is None:
        channels = 1 if a.ndim == 2 else 3
    H, W = a.shape[:2]
    hist = {}

    def count(key, n=1):
        hist[key] = hist.get(key, 0) + n

    planes = _samples(a, channels)
    q = quant_tables(quality)
    dc = [huffman(DC_BITS[s], DC_VALS) for s in range(2)]
    ac = [huffman(AC_BITS[s], AC_VALS[s]) for s in range(2)]
    bw, bh = (W + 7) // 8, (H + 7) // 8
    out = bytearray(header(W, H, channels, quality, restart_rows))
    n_int = (bh + restart_rows - 1) // restart_rows
    for i in range(n_int):
        bits = _Bits()
        pred = [0] * channels
        for by in range(i * restart_rows, min(bh, (i + 1) * restart_rows)):
            for bx in range(bw):
                for c in range(channels):
                    s = 1 if c else 0
                    block = [[planes[c][min(8 * by + y, H - 1)][min(8 * bx + x, W - 1)] for x in range(8)] for y in range(8)]
                    co = fdct(block)
                    zz = []
                    for k in range(64):
                        v, u = divmod(ZIGZAG[k], 8)
                        cv, qv = co[v][u], q[s][ZIGZAG[k]]
                        m = (2 * abs(cv) + COEF_ONE * qv) // (2 * COEF_ONE * qv)     # cv is 8 c: (2|c| + q) // (2q)
                        zz.append(-m if cv < 0 else m)
                    diff = zz[0] - pred[c]
                    pred[c] = zz[0]
                    cat = _category(diff)
                    count("dc%d" % cat)
                    bits.put(*dc[s][cat])
                    bits.value(diff, cat)
                    run = 0
                    for k in range(1, 64):
                        if zz[k] == 0:
                            run += 1
                            continue
                        while run > 15:
                            bits.put(*ac[s][0xF0])
                            count("zrl")
                            run -= 16
                        size = _category(zz[k])
                        count("ac%d" % size)
                        bits.put(*ac[s][(run << 4) | size])
                        bits.value(zz[k], size)
                        run = 0
                    if run > 0:
                        bits.put(*ac[s][0x00])
                        count("eob")
                    else:
                        count("no_eob")
        data = bits.stuffed()
        count("stuffed", data.count(b"\xff\x00"))
        count("intervals")
        out += data
        out += bytes([0xFF, 0xD9 if i == n_int - 1 else 0xD0 + (i & 7)])
    return bytes(out), hist


# ---- the frames both test files use ----------------------------------------------------------------------------------
def _noise(W, H, channels, seed):
    shape = (H, W, 3) if channels == 3 else (H, W)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth_image(W, H, channels=3):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = [127.5 + 100 * np.sin(x / 9.0 + p) * np.cos(y / 7.0 - p) + 20 * np.sin((x + y) / 3.0) for p in (0.0, 1.0, 2.0)]
    a = np.clip(np.rint(np.stack(planes, 2)), 0, 255).astype(np.uint8)
    return a if channels == 3 else np.ascontiguousarray(a[:, :, 0])


def _blocks(W, H, block):
    """a grey frame whose 8x8 block (bx, by) is block(bx, by)"""
    a = np.zeros((H, W), np.uint8)
    for by in range(H // 8):
        for bx in range(W // 8):
            a[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = block(bx, by)
    return a


def _basis77():
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return np.clip(np.rint(128 + 120 * np.outer(c, c)), 0, 255).astype(np.uint8)


def cases():
    """[(name, frame, quality, restart_rows)]: the smallest shapes at which the encoder can go wrong.  Sizes are W x H."""
    out = []
    for W, H in ((1, 1), (7, 9), (8, 8), (9, 8), (61, 45)):               # block edges and padding
        for ch in (1, 3):
            f = smooth_image(W, H, ch).astype(np.int16) + _noise(W, H, ch, W + ch).astype(np.int16) % 41 - 20
            out.append(("edge_%dx%d_c%d" % (W, H, ch), np.clip(f, 0, 255).astype(np.uint8), 90, 1))
    out.append(("restart_24x80_r1", _noise(24, 80, 3, 1), 75, 1))          # ten intervals: RST7 is followed by RST0
    out.append(("restart_24x80_r3", _noise(24, 80, 3, 1), 75, 3))          # the last interval has one row
    out.append(("wide_520x8_c1", _noise(520, 8, 1, 2), 90, 1))             # 65 blocks in an interval
    out.append(("wide_520x8_c3", _noise(520, 8, 3, 3), 90, 1))             # 195
    out.append(("wide_2056x8_c1", _noise(2056, 8, 1, 4), 90, 1))           # 257
    out.append(("wide_2056x16_r2", _noise(2056, 16, 1, 5), 90, 2))         # 514 in one interval
    # more blocks in an interval than the 1024 threads its workgroup has at most: a second, partial turn (1542 = 1024 +
    # 518; the DC prediction of block 1024 comes from the turn before), and one block into the second turn (1025)
    out.append(("turns_2056x16_c3_r2", _noise(2056, 16, 3, 7), 90, 2))
    out.append(("turns_8200x8_c1", _noise(8200, 8, 1, 8), 75, 1))
    out.append(("tall_8x2056_c1", _noise(8, 2056, 1, 9), 75, 1))           # 257 intervals: a second turn of the offsets' scan
    out.append(("dc11", _blocks(32, 16, lambda bx, by: 255 * ((bx + by) & 1)), 100, 1))
    half = np.zeros((8, 8), np.uint8)
    half[:, 4:] = 255
    out.append(("ac10", _blocks(32, 16, lambda bx, by: half if (bx + by) & 1 else half.T), 100, 1))
    out.append(("noise_q100", _noise(40, 24, 3, 6), 100, 1))
    out.append(("basis77_q50", _blocks(24, 8, lambda bx, by: _basis77()), 50, 1))
    return out


_reference = {}


def reference(name):
    """(file bytes, histogram) of a case, computed once"""
    if name not in _reference:
        for n, frame, q, rr in cases():
            if n == name:
                _reference[name] = encode(frame, q, rr)
    return _reference[name]
