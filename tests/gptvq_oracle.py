"""numpy oracle of the two GPTVQ kernels (aimet_amd/csrc/gptvq.hip), in the kernels' fp32 operation
order: every product, sum and divide is one numpy float32 operation, so each is rounded on its own.

* dist(x, c) = sum over d ascending of (x_d - c_d) * (x_d - c_d); the assignment is the first minimum.
* kmeans_step: the assignments bit for bit, the means in float64 (the kernel's sum over a cluster is a
  long fp32 sum in a fixed order of its own; the tests bound the difference).
* block_update: the sweep inside one column block, bit for bit.
"""
import numpy as np

F32 = np.float32


def sq_dist(x, c):
    """x [..., D], c [K, D] -> [..., K] float32."""
    x = np.asarray(x, F32)
    c = np.asarray(c, F32)
    diff = x[..., None, :] - c
    sq = diff * diff
    acc = sq[..., 0]
    for d in range(1, sq.shape[-1]):
        acc = acc + sq[..., d]
    assert acc.dtype == F32
    return acc


def assign(x, c):
    """First minimum over the centroids (np.argmin returns the first occurrence)."""
    return np.argmin(sq_dist(x, c), axis=-1).astype(np.int32)


def group_vectors(w_block, rows_per_block, D):
    """[rows][ncols] -> [G][N][D]: vector n = r * (ncols / D) + t of a group."""
    rows, ncols = w_block.shape
    return np.ascontiguousarray(w_block, F32).reshape(rows // rows_per_block, rows_per_block * ncols // D, D)


def kmeans_step(x, codebook):
    """One Lloyd step from `codebook` [G][K][D] on x [G][N][D]: (new codebook in float64, assignments,
    counts [G][K], sum of |x| per (g, k, d) in float64)."""
    G, K, D = codebook.shape
    new = np.zeros((G, K, D), np.float64)
    mags = np.zeros((G, K, D), np.float64)
    counts = np.zeros((G, K), np.int64)
    assigns = np.empty(x.shape[:2], np.int32)
    for g in range(G):
        a = assign(x[g], codebook[g])
        assigns[g] = a
        counts[g] = np.bincount(a, minlength=K)
        for d in range(D):
            new[g, :, d] = np.bincount(a, weights=x[g, :, d].astype(np.float64), minlength=K)
            mags[g, :, d] = np.bincount(a, weights=np.abs(x[g, :, d]).astype(np.float64), minlength=K)
        new[g] /= np.maximum(counts[g], 1)[:, None]
    return new, assigns, counts, mags


def kmeans(x, codebook, iterations):
    """`iterations` Lloyd steps, each mean computed in float64 and rounded to fp32."""
    codebook = np.array(codebook, F32)
    for _ in range(iterations):
        codebook = kmeans_step(x, codebook)[0].astype(F32)
    return codebook


def block_update(w, rows_per_block, b0, s0, s1, block_end, D, codebook, hinv, err, indices):
    """aimet_gptvq_block_update on numpy arrays, in place: w [rows][cols], codebook [G][K][D],
    hinv [cols][cols], err [rows][block_end - b0], indices [rows][(block_end - b0) / D]."""
    assert w.dtype == F32 and codebook.dtype == F32 and hinv.dtype == F32 and err.dtype == F32
    rows = w.shape[0]
    group = np.arange(rows) // rows_per_block
    for i in range(s0, s1, D):
        c = b0 + i
        x = w[:, c:c + D].copy()
        k = np.empty(rows, np.int32)
        for g in range(codebook.shape[0]):
            sel = group == g
            k[sel] = assign(x[sel], codebook[g])
        q = codebook[group, k]
        diag = np.array([hinv[c + d, c + d] for d in range(D)], F32)
        e = (x - q) / diag
        assert e.dtype == F32
        w[:, c:c + D] = q
        if c + D < block_end:
            upd = e[:, 0:1] * hinv[c, c + D:block_end][None, :]
            for d in range(1, D):
                upd = upd + e[:, d:d + 1] * hinv[c + d, c + D:block_end][None, :]
            assert upd.dtype == F32
            w[:, c + D:block_end] = w[:, c + D:block_end] - upd
        err[:, i:i + D] = e
        indices[:, i // D] = k
