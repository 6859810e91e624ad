"""hydra_mi.pca restated in loops and Python integers: the Gram matrix of frames, its centring, the
components, the frame similarity and the frame score, and the figures of the planted video with ensembles
(network_ref.planted_video).  tests/test_pca_cpu.py and tests/test_pca_gpu.py compare the two bit for bit."""
import math

import numpy as np

import network_ref


def gram(frames):
    """frames (F, ...) uint8 -> (G (F, F) int64, s1 (F,) uint64).  The products are made by the float64 matrix product,
    which is exact here: every partial sum is a whole number of at most 65025 x pixels, asserted below 2^53."""
    X = np.asarray(frames)
    assert X.dtype == np.uint8
    X = X.reshape(X.shape[0], -1)
    assert 65025 * X.shape[1] < 1 << 53
    Xd = X.astype(np.float64)
    G = (Xd @ Xd.T).astype(np.int64)
    return G, X.astype(np.uint64).sum(1)


def gram_loops(frames):
    """the same by int64 products of every pair of frames: what the small cases check `gram` against"""
    X = np.asarray(frames).reshape(len(frames), -1).astype(np.int64)
    F = X.shape[0]
    G = np.empty((F, F), np.int64)
    for i in range(F):
        for j in range(F):
            G[i, j] = int((X[i] * X[j]).sum())
    return G, X.sum(1).astype(np.uint64)


def centre(G):
    F = len(G)
    g = [[int(v) for v in row] for row in G]
    r = [sum(row) for row in g]
    t = sum(r)
    out = np.empty((F, F), np.float64)
    for i in range(F):
        for j in range(F):
            out[i, j] = np.float64(float(F * F * g[i][j] - F * r[i] - F * r[j] + t)) / np.float64(float(F * F))
    return out


def components(G, k):
    """the eigenvectors are LAPACK's (numpy.linalg.eigh of the restated centre); the order, the clip and the sign rule are
    restated"""
    Gc = centre(G)
    w, V = np.linalg.eigh(Gc)
    F = len(w)
    lam, U, share = np.empty(k), np.empty((F, k)), np.empty(k)
    tr = np.trace(Gc)
    for c in range(k):
        col = V[:, F - 1 - c]
        lam[c] = w[F - 1 - c] if w[F - 1 - c] > 0.0 else 0.0
        big = 0
        for f in range(F):
            if abs(col[f]) > abs(col[big]):
                big = f
        U[:, c] = -col if col[big] < 0.0 else col
        with np.errstate(invalid="ignore", divide="ignore"):
            share[c] = lam[c] / tr
    return lam, U, share


def frame_similarity(G, s1, npix):
    F = len(G)
    C = [[npix * int(G[i][j]) - int(s1[i]) * int(s1[j]) for j in range(F)] for i in range(F)]
    r = np.full((F, F), np.nan)
    for i in range(F):
        for j in range(F):
            if C[i][i] != 0 and C[j][j] != 0:
                r[i, j] = np.float64(float(C[i][j])) / np.sqrt(np.float64(float(C[i][i])) * np.float64(float(C[j][j])))
    return r


def frame_score(r):
    F = len(r)
    out = np.full(F, np.nan)
    for i in range(F):
        x = sorted(float(r[i][j]) for j in range(F) if j != i and not math.isnan(r[i][j]))
        m = len(x)
        if m:
            out[i] = x[m // 2] if m % 2 else (x[m // 2 - 1] + x[m // 2]) / 2.0
    return out


def maps(frames, inmap, U):
    """every component's correlation image: network_ref.maps of the temporal vectors (F, k) as traces"""
    return network_ref.maps(frames, inmap, np.asarray(U, np.float64).T)


# ---- the planted video with ensembles -------------------------------------------------------------------------------
def r_squared(y, X):
    """R^2 of the least-squares fit of y (F,) on a constant and the columns of X (F, K)"""
    A = np.concatenate((np.ones((len(y), 1)), X), 1)
    res = y - A @ np.linalg.lstsq(A, y, rcond=None)[0]
    d = y - y.mean()
    return 1.0 - float(res @ res) / float(d @ d)


def planted_neuropil(video, centres, far=10):
    """The planted neuropil as the video shows it: per frame the mean of the pixels more than `far` px from every planted
    centre.  There a cell adds at most 50 exp(-far^2 / (2 x 2.5^2)) = 0.017 grey levels, the texture is constant over time
    and the noise of -8..8 averages out over thousands of pixels: what is left moves with the neuropil alone."""
    H, W = video.shape[1:]
    yy, xx = np.mgrid[0:H, 0:W]
    keep = np.ones((H, W), bool)
    for cx, cy in centres:
        keep &= (xx - cx) ** 2 + (yy - cy) ** 2 > far * far
    return video[:, keep].astype(np.float64).mean(1)


def planted_figures(seed):
    """PCA of the raw planted video with ensembles -> dict: share (5,), r2 {K: the lowest R^2 of the three ensembles' mean
    activity on a constant and the first K temporal vectors} for K 3 and 4, npil (4,): |Pearson's r| of each of the first
    four temporal vectors with the planted neuropil"""
    v, cs, act = network_ref.planted_video(seed)
    G, _ = gram(v)
    lam, U, share = components(G, 5)
    ens = [act[[i for i in range(len(act)) if network_ref.planted_ensemble(i) == e]].mean(0) for e in range(network_ref.ENSEMBLES["E"])]
    r2 = {K: min(r_squared(y, U[:, :K]) for y in ens) for K in (3, 4)}
    n = planted_neuropil(v, cs)
    npil = np.array([abs(np.corrcoef(U[:, c], n)[0, 1]) for c in range(4)])
    return dict(share=share, r2=r2, npil=npil)
