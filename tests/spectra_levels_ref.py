"""The definition of x3_spectra_levels_dev (include/x3hip.h, "SPECTRA, BAND LEVELS") in numpy (not a test module), built on
spectra_ref.py.  Integers only.

The rule (N, H, table), B = N / 2 + 1, R = spectra_ref.n_rows and the POWER word ms[r][k] = spectra_ref.power are the rows
call's.  A fold is (M = frames_per_bin in 1 .. 2^31 - 1, K = n_bands in 1 .. B, bin_band: B uint32 words, a word >= K: no
band).  A row of R frames has T = ceil(R / M) time bins, time bin j the frames [j * M, min((j + 1) * M, R)); for band b
    bp[r][b] = min(2^30, sum over k with bin_band[k] == b of ms[r][k])
and the record of (j, b) is n = the frames of the bin, sum_sq = the sum of their bp, sum = 0, max = min(32767, isqrt(2 * the
largest bp)), min = -max, reserved = 0; the identity (0, 0, 32767, -32768, 0, 0) where no frame falls.

spectra_levels is a whole call: K planes of records, plane b at b * plane_stride, the rows laid by spectra_ref.spectra_rows'
rules with T for R."""
import numpy as np

import spectra_ref as S

ERR_BAD_ARG = S.ERR_BAD_ARG
LEVEL = np.dtype([("sum_sq", np.uint64), ("sum", np.int64), ("min", np.int32), ("max", np.int32), ("n", np.uint32),
                  ("reserved", np.uint32)])
IDENTITY = np.array([(0, 0, 32767, -32768, 0, 0)], dtype=LEVEL)[0]
CLAMP = 1 << 30


def n_bins_of(rows, per_bin):
    """T of a row of `rows` frames"""
    return -(-rows // per_bin)


def band_power(ms, bin_band, n_bands):
    """uint32 [R, B] POWER words -> int64 [R, K]: the frames' clamped band sums"""
    ms = np.asarray(ms).astype(np.int64)
    bp = np.zeros((ms.shape[0], n_bands), dtype=np.int64)
    for k, b in enumerate(np.asarray(bin_band, dtype=np.uint32).tolist()):
        if b < n_bands:
            bp[:, b] += ms[:, k]
    return np.minimum(bp, CLAMP)


def fold_rows(ms, per_bin, bin_band, n_bands):
    """uint32 [R, B] POWER words of one row -> LEVEL [K, T]"""
    bp = band_power(ms, bin_band, n_bands)
    r = bp.shape[0]
    t = n_bins_of(r, per_bin)
    out = np.zeros((n_bands, t), dtype=LEVEL)
    if t == 0:
        return out
    per_bin = min(per_bin, r)                                  # (one bin then: nothing is padded up to 2^31 frames)
    full = np.zeros((t * per_bin, n_bands), dtype=np.int64)    # (bp >= 0: frames of zeros change neither sum nor max)
    full[:r] = bp
    full = full.reshape(t, per_bin, n_bands)
    peak = np.minimum(isqrt(2 * full.max(axis=1)), 32767)
    out["sum_sq"] = full.sum(axis=1).T                         # (at most 2^31 frames of 2^30)
    out["max"], out["min"] = peak.T, -peak.T
    out["n"] = np.minimum(per_bin, r - per_bin * np.arange(t))[None, :]
    return out


def isqrt(v):
    """floor square roots of an int64 array of values below 2^32"""
    v = np.asarray(v, dtype=np.int64)
    s = np.sqrt(v.astype(np.float64)).astype(np.int64)
    s -= s * s > v
    s += (s + 1) * (s + 1) <= v
    assert ((s * s <= v) & ((s + 1) * (s + 1) > v)).all()
    return s


def levels_of(x, n_fft, hop, per_bin, bin_band, n_bands, tab=None):
    """LEVEL [K, T] of the row x"""
    return fold_rows(S.power(x, n_fft, hop, tab), per_bin, bin_band, n_bands)


def spectra_levels(samples, offsets, lens, in_status, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap, plane_stride=0,
                   tab=None, fill=0x5A, powers=None):
    """x3_spectra_levels_dev on host arrays -> (levels LEVEL [K, plane_stride or rows_cap], row_offsets uint64 [n + 1], status
    int32 [n], total time bins); what the call does not write keeps the byte `fill`.  ValueError where the call is refused.
    powers: None, or a dict that keeps spectra_ref.power of a range under (offset, length) from one call to the next (the
    same samples, rule and table)."""
    samples = np.asarray(samples, dtype=np.int16)
    bin_band = np.asarray(bin_band, dtype=np.uint32)
    n, cap_s, nb = len(lens), len(samples), S.n_bins(n_fft)
    if (n_fft not in S.NFFTS or not 1 <= hop <= 0x7FFFFFFF or not 1 <= per_bin <= 0x7FFFFFFF or not 1 <= n_bands <= nb
            or bin_band.shape != (nb,) or (plane_stride and plane_stride < rows_cap)
            or n_bands * max(plane_stride, rows_cap) > 0x7FFFFFFF or not 1 <= n <= 0x7FFFFFFF
            or not 1 <= rows_cap <= 0x7FFFFFFF or (stride and n * stride > rows_cap)):
        raise ValueError("refused")
    ps = plane_stride or rows_cap
    out = np.full(n_bands * ps * LEVEL.itemsize, fill, dtype=np.uint8).view(LEVEL).reshape(n_bands, ps)
    bins = [n_bins_of(S.n_rows(int(l), n_fft, hop), per_bin) for l in lens]
    off = np.zeros(n + 1, dtype=np.uint64)
    run = np.concatenate([[0], np.cumsum(np.asarray(bins, dtype=np.int64))])
    status = np.zeros(n, dtype=np.int32)
    for w in range(n):
        t, o, l = bins[w], int(offsets[w]), int(lens[w])
        base = w * stride if stride else int(run[w])
        off[w] = base
        fits = (t <= stride) if stride else (base + t <= rows_cap)
        st = int(in_status[w]) if in_status is not None else 0
        if st == 0 and o + l > cap_s:
            st = ERR_BAD_ARG
        if st == 0 and not fits:
            st = ERR_BAD_ARG
        status[w] = st
        if stride:
            out[:, base:base + stride] = IDENTITY
        else:
            out[:, base:min(base + t, rows_cap)] = IDENTITY   # (rows [0, min(total, rows_cap)) are the call's)
        if st == 0 and t:
            ms = powers.get((o, l)) if powers is not None else None
            if ms is None:
                ms = S.power(samples[o:o + l], n_fft, hop, tab)
                if powers is not None:
                    powers[(o, l)] = ms
            out[:, base:base + t] = fold_rows(ms, per_bin, bin_band, n_bands)
    off[n] = n * stride if stride else int(run[n])
    return out, off, status, int(run[n])
