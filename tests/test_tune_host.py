"""Parameter tuning without a GPU (include/x3hip.h, "parameter tuning"): the candidate grid of x3_tune_candidate against a
restatement of the rules that make a set safe, the argument checks, and the tuning kernel's resources."""
import os
import re
import subprocess

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = x3hip.ERR_BAD_ARG


def _rice(c):
    """RiceCodes (src/x3.rs:187-260) as the library exports them: (offset, table length) of code c"""
    rc_ = x3hip.RiceCode()
    assert x3hip.lib().x3_rice_code_get(c, x3hip.C.byref(rc_)) == 0
    return rc_.offset, rc_.len


def stream_safe(codes, thr):
    """x3_encode.hip's stream_safe_thresholds: every code in use holds every difference that can reach it"""
    mmax, used = [0, 0, 0], [False] * 3
    for m in range(min(thr[2], 70000) + 1):
        ft = (m > thr[0]) + (m > thr[1])
        used[ft], mmax[ft] = True, m
    for ft in range(3):
        if used[ft]:
            c = codes[ft]
            if c > 3:
                return False
            off, ln = _rice(c)
            if mmax[ft] > min(off, ln - off - 1):
                return False
    return True


def safe_sets():
    """every set the rules allow: codes (0, 1, 3), single-pass block lengths, t2 >= 15, stream-safe, t0 <= t1"""
    out = []
    for bl in (10, 20, 40):
        for t0 in range(0, 32):
            for t1 in range(t0, 32):
                for t2 in range(15, 64):
                    if stream_safe((0, 1, 3), (t0, t1, t2)):
                        out.append((bl, t0, t1, t2))
    return out


def test_candidates_are_exactly_the_safe_sets_in_index_order():
    for spf in (40, 10000, 10240):
        got = []
        for i in range(x3hip.TUNE_CANDIDATES):
            rc, p = x3hip.tune_candidate(i, spf)
            assert rc == 0, (i, spf)
            assert list(p.codes) == [0, 1, 3]
            assert p.block_len * p.blocks_per_frame == spf
            t = tuple(p.thresholds)
            assert t[2] >= 15 and t[0] <= t[1] and stream_safe((0, 1, 3), t)
            assert x3hip.lib().x3_params_validate(x3hip.C.byref(p)) == 0
            got.append((p.block_len,) + t)
        assert got == safe_sets(), spf    # the same sets, in the documented order (g * 728 + lexicographic rank)
        assert len(got) == 2184 and len(set(got)) == 2184
    rc, p = x3hip.tune_candidate(x3hip.TUNE_DEFAULT_INDEX)
    d = x3hip.Params.default()
    assert (p.block_len, p.blocks_per_frame, list(p.thresholds)) == (d.block_len, d.blocks_per_frame, list(d.thresholds))


def test_grid_limits_are_the_stream_safe_edges():
    # one step past each limit is not stream-safe: t0 = 7, t1 = 11, t2 = 28
    assert not stream_safe((0, 1, 3), (7, 8, 20))
    assert not stream_safe((0, 1, 3), (3, 11, 20))
    assert not stream_safe((0, 1, 3), (3, 8, 28))
    assert stream_safe((0, 1, 3), (6, 10, 27))


def test_bad_spf_and_index():
    for spf in (0, 30, 39, 41, 10000 + 20, 10280, 20000, 1 << 31):
        assert x3hip.tune_candidate(0, spf)[0] == BAD, spf
    for i in (2184, 2185, 1 << 31):
        assert x3hip.tune_candidate(i, 10000)[0] == BAD, i
    assert x3hip.lib().x3_tune_candidate(0, 10000, None) == BAD
    # entry points that need a tuner or a context refuse NULL without touching the GPU
    L = x3hip.lib()
    assert L.x3_tuner_create(None, 10000, x3hip.C.byref(x3hip.C.c_void_p())) == BAD
    assert L.x3_tuner_add_dev(None, None, None) == BAD
    assert L.x3_tuner_result(None, None, None, None) == BAD
    assert L.x3_tuner_reset(None) == BAD
    assert L.x3_tune(None, None, 0, 10000, None, None, None) == BAD
    L.x3_tuner_destroy(None)


def test_tune_kernel_uses_no_scratch(tmp_path):
    """the tuning kernel keeps its 96 sums per lane in registers: no spill to scratch"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "x3-rust_amd", "csrc", "x3_tune.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o",
                        str(tmp_path / "t.o"), src, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = r.stderr
    at = txt.find("Function Name: _Z14x3_tune_kernel")
    assert at >= 0, txt[-2000:]
    block = txt[at:at + 2000]
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block), block
    assert re.search(r"VGPRs Spill: 0\b", block), block
    assert re.search(r"SGPRs Spill: 0\b", block), block
