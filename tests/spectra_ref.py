"""The definition of x3_spectra_rows_dev (include/x3hip.h, "SPECTRA") in numpy (not a test module).  Integers only.

A rule is (n_fft = N in NFFTS, hop = H >= 1, a table of 1 024 (cos, sin) int16 pairs); B = N / 2 + 1 bins.  For a row of
len int16 samples: R = 0 when len < N, else (len - N) // H + 1 frames -- whole frames only -- frame r is
x[r * H : r * H + N], and bin k of it is
    re = sum over n < N of x[r * H + n] * cos[((n * k) mod N) * (1024 / N)],   im = the same against sin
in int64, exact.  The oscillator restarts at every frame.  SUMS rows are [B, 2] int64; POWER rows are [B] uint32, each
the tone adapter's ms at n = N: a = re >> 15, b = im >> 15, P = a * a + b * b, ms = min(2^30, (2 * P // N) // N).

The statuses and layouts of a call: spectra_rows.  split_model is the kernels' arithmetic -- every int16 as two int8 and
the epilogue that puts the four 8-bit products together -- which must equal the definition on every input."""
import numpy as np

import tone_levels_ref as TL

ERR_BAD_ARG = 24
SUMS, POWER = 0, 1
NFFTS = (64, 128, 256, 512, 1024)
PAIRS = TL.PAIRS
table = TL.table


def n_bins(n_fft):
    return n_fft // 2 + 1


def n_rows(length, n_fft, hop):
    """R of a row of `length` samples"""
    return 0 if length < n_fft else (length - n_fft) // hop + 1


def basis(n_fft, tab=None):
    """int64 [N, B, 2]: the table pair of (n, k)"""
    assert n_fft in NFFTS
    tab = table() if tab is None else np.asarray(tab, dtype=np.int16).reshape(PAIRS, 2)
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_bins(n_fft), dtype=np.int64)[None, :]
    return tab[((n * k) % n_fft) * (PAIRS // n_fft)].astype(np.int64)


def frames_of(x, n_fft, hop):
    """int64 [R, N]: the whole frames of row x"""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    r = n_rows(len(x), n_fft, hop)
    if r == 0:
        return np.zeros((0, n_fft), dtype=np.int64)
    return x[np.arange(r, dtype=np.int64)[:, None] * hop + np.arange(n_fft, dtype=np.int64)[None, :]]


def sums(x, n_fft, hop, tab=None):
    """int64 [R, B, 2] of row x.  (|x * c| <= 2^30 and N <= 2^10 terms: int64 never wraps)"""
    fr = frames_of(x, n_fft, hop)
    return np.einsum("rn,nkc->rkc", fr, basis(n_fft, tab))


def power_of(s, n_fft):
    """int64 [..., 2] sums -> uint32 [...]: the adapter's ms with n = N"""
    a, b = s[..., 0] >> 15, s[..., 1] >> 15   # (numpy's >> on int64 is the arithmetic shift)
    p = a * a + b * b                         # (below 2^51)
    return np.minimum((2 * p // n_fft) // n_fft, 1 << 30).astype(np.uint32)


def power(x, n_fft, hop, tab=None):
    return power_of(sums(x, n_fft, hop, tab), n_fft)


def split(v):
    """int16 values -> (vh, vl), int64 arrays holding int8 values, with v = 256 * vh + vl + 128"""
    v = np.asarray(v).astype(np.int64)
    vh, vl = v >> 8, (v & 255) - 128
    assert vh.min(initial=0) >= -128 and vh.max(initial=0) <= 127 and vl.min(initial=0) >= -128 and vl.max(initial=0) <= 127
    return vh, vl


def split_model(x, n_fft, hop, tab=None):
    """sums() the kernels' way: four 8-bit products in int32, the frame's and the column's sums, the epilogue in int64"""
    fr = frames_of(x, n_fft, hop)
    bs = basis(n_fft, tab)
    xh, xl = split(fr)
    ch, cl = split(bs)
    prod = lambda a, b: np.einsum("rn,nkc->rkc", a, b)
    hh, hl, lh, ll = prod(xh, ch), prod(xh, cl), prod(xl, ch), prod(xl, cl)
    for acc in (hh, hl, lh, ll):   # (what an int32 accumulator holds: N * 2^14 <= 2^24 at most)
        assert np.abs(acc).max(initial=0) <= n_fft << 14
    sx = (256 * xh + xl).sum(axis=1)[:, None, None]
    sc = (256 * ch + cl).sum(axis=0)[None, :, :]
    return 65536 * hh + 256 * (hl + lh) + ll + 128 * sx + 128 * sc + 16384 * n_fft


def spectra_rows(samples, offsets, lens, in_status, n_fft, hop, fmt, stride, rows_cap, tab=None, fill=0x5A):
    """x3_spectra_rows_dev on host arrays -> (out, row_offsets uint64 [n + 1], status int32 [n], total rows).
    samples: int16 [samples_cap]; in_status: None or int32 [n]; stride 0: packed.  out is [rows_cap, B, 2] int64 (SUMS)
    or [rows_cap, B] uint32 (POWER); what the call does not write keeps the byte `fill`.  ValueError where the call is
    refused."""
    samples = np.asarray(samples, dtype=np.int16)
    n, cap_s, nb = len(lens), len(samples), n_bins(n_fft)
    if (n_fft not in NFFTS or not 1 <= hop <= 0x7FFFFFFF or fmt not in (SUMS, POWER) or not 1 <= n <= 0x7FFFFFFF
            or not 1 <= rows_cap <= 0x7FFFFFFF or (stride and n * stride > rows_cap)):
        raise ValueError("refused")
    out = (np.full(rows_cap * nb * (16 if fmt == SUMS else 4), fill, dtype=np.uint8)
           .view(np.int64 if fmt == SUMS else np.uint32).reshape((rows_cap, nb, 2) if fmt == SUMS else (rows_cap, nb)))
    rows = [n_rows(int(l), n_fft, hop) for l in lens]
    off = np.zeros(n + 1, dtype=np.uint64)
    run = np.concatenate([[0], np.cumsum(np.asarray(rows, dtype=np.int64))])
    status = np.zeros(n, dtype=np.int32)
    for w in range(n):
        r, o, l = rows[w], int(offsets[w]), int(lens[w])
        base = w * stride if stride else int(run[w])
        off[w] = base
        fits = (r <= stride) if stride else (base + r <= rows_cap)
        st = int(in_status[w]) if in_status is not None else 0
        if st == 0 and o + l > cap_s:
            st = ERR_BAD_ARG
        if st == 0 and not fits:
            st = ERR_BAD_ARG
        status[w] = st
        if stride:
            out[base:base + stride] = 0
        elif fits:
            out[base:base + r] = 0
        if st == 0 and r:
            s = sums(samples[o:o + l], n_fft, hop, tab)
            out[base:base + r] = s if fmt == SUMS else power_of(s, n_fft)
    off[n] = n * stride if stride else int(run[n])
    return out, off, status, int(run[n])
