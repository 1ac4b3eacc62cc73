"""numpy restatement of the three PointNet++ adjoints of include/t2h_pnpp.h (t2h_group_max_bwd, t2h_index_transpose,
t2h_rows_gather_bwd) with the header's exact fp32 operations and association, plus float64 versions and the summation bound.

    group max:  per group and column the LOWEST row with rows[j, c] - out[c] == 0 (fp32) takes gout[c]; +0 elsewhere, in the
                columns C .. gld, and (relu) in every column with NOT (out[c] > 0)
    transpose:  offsets / entries = the CSR of idx by value, each segment in ascending position; an index outside [0, n) counts
                as n - 1
    gather:     chunks of CHUNK = 64 consecutive entries of a segment, each summed from +0 in ascending order (term = w * g
                rounded, then added; an entry with w == 0 adds nothing); lane sum y of LANES = 4 adds the chunk sums k = y, y + 4,
                ... from +0 in ascending k; out = ((lane_0 + lane_1) + lane_2) + lane_3
Single clouds; the callers loop over the batch.
"""
import numpy as np

F = np.float32
CHUNK, LANES = 64, 4          # T2H_GATHER_CHUNK, T2H_GATHER_LANES


def group_max_bwd(rows, nsample, out, gout, relu, gld=None):
    """rows [groups * nsample, ld], out / gout [groups, C] -> grows [groups * nsample, gld] float32."""
    rows, out, gout = np.asarray(rows, F), np.asarray(out, F), np.asarray(gout, F)
    groups, c = out.shape
    gld = c if gld is None else gld
    grows = np.zeros((groups, nsample, gld), F)
    r = rows.reshape(groups, nsample, -1)[:, :, :c]
    with np.errstate(invalid="ignore"):
        hit = (r - out[:, None, :]) == F(0)                          # fp32 subtraction: NaN and inf - inf match nothing
    first = np.where(hit.any(1), hit.argmax(1), -1)                  # [groups, C]: the lowest matching row
    gv = gout.copy()
    if relu:
        gv[~(out > 0)] = F(0)
    gi, ci = np.nonzero(first >= 0)
    grows[gi, first[gi, ci], ci] = gv[gi, ci]
    return grows.reshape(groups * nsample, gld)


def index_transpose(idx, n):
    """idx: any shape, int -> (offsets [n + 1] int32, entries [E] int32)."""
    flat = np.asarray(idx).reshape(-1).astype(np.int64)
    flat = np.where((flat < 0) | (flat >= n), n - 1, flat)
    offsets = np.zeros(n + 1, np.int32)
    entries = np.empty(flat.size, np.int32)
    pos = 0
    for i in range(n):
        e = np.flatnonzero(flat == i)                                 # (ascending)
        entries[pos:pos + e.size] = e
        pos += e.size
        offsets[i + 1] = pos
    return offsets, entries


def index_cases():
    """(idx, n) of the transpose tests: a source that is never referenced (13), one referenced more than four chunk lengths of
    times (21), the empty-group marker n; [7, 5] and [1100] over 70 sources, and 390 references of a single source."""
    rng = np.random.default_rng(5)
    small = rng.integers(0, 70, (7, 5))
    small[small == 13] = 14
    small[2, 3] = 70
    big = rng.integers(0, 70, 1100)
    big[big == 13] = 12
    big[rng.choice(1100, 300, replace=False)] = 21
    big[[5, 700]] = 70
    return [(small, 70), (big, 70), (np.zeros(390, np.int64), 1)]


def rows_gather_bwd(g, col0, d, weight, fan, offsets, entries, n):
    """g [E / fan, gld] float32, weight [E] (any shape) or None -> out [n, d] float32 in the header's association."""
    g = np.asarray(g, F)
    w_all = None if weight is None else np.asarray(weight, F).reshape(-1)
    out = np.zeros((n, d), F)
    for i in range(n):
        seg = entries[offsets[i]:offsets[i + 1]].astype(np.int64)
        lanes = np.zeros((LANES, d), F)
        for k in range(0, -(-seg.size // CHUNK)):
            p = np.zeros(d, F)
            for e in seg[k * CHUNK:(k + 1) * CHUNK]:
                v = g[e // fan, col0:col0 + d]
                if w_all is None:
                    p = p + v
                elif w_all[e] != 0:
                    p = p + w_all[e] * v                              # (numpy rounds the product, then the sum)
            lanes[k % LANES] = lanes[k % LANES] + p
        t = lanes[0]
        for y in range(1, LANES):
            t = t + lanes[y]
        out[i] = t
    return out


def rows_gather_bwd64(g, col0, d, weight, fan, offsets, entries, n):
    """-> (float64 sums [n, d], bound [n, d]): |fp32 result - float64 sum| <= ((m - 1) + 1) * 2^-24 * sum|terms| for a segment of m
    non-skipped terms in ANY order of summation (m - 1 additions of relative error 2^-24 each, to first order, plus the
    rounding of each product)."""
    g = np.asarray(g, np.float64)
    w_all = None if weight is None else np.asarray(weight, np.float64).reshape(-1)
    out, bound = np.zeros((n, d)), np.zeros((n, d))
    for i in range(n):
        seg = entries[offsets[i]:offsets[i + 1]].astype(np.int64)
        terms = g[seg // fan, col0:col0 + d]
        if w_all is not None:
            keep = w_all[seg] != 0
            terms = terms[keep] * w_all[seg][keep, None]
        m = terms.shape[0]
        out[i] = terms.sum(0)
        bound[i] = ((max(m - 1, 0) + (0 if w_all is None else 1)) * 2.0 ** -24) * np.abs(terms).sum(0)
    return out, bound
