"""The asynchronous contract of the analysis calls (include/x3hip.h: "Asynchronous on the context's stream: one launch set,
no host trip"): levels, events, quantiles, thresholds, range levels and x3_corpus_ranges_dev, in their stream and corpus
forms.  A C, C++ or Rust caller who chains these calls on a busy stream is the one who would meet an ordering bug; the
Python classes wait in front of and behind every call and never see the GPU lag.

A  every call, and the chain levels -> thresholds -> events -> range levels -> ranges, behind a stalled stream with its
   inputs arriving behind the stall (async_analysis_cases.py, through async_cases.run_stalled)
B  two host threads, a context each, one shared corpus
C  the host structs (x3_level_fir, x3_event_rule, x3_threshold_rule) are read at the call
Every comparison is == against the CPU references; no test asserts a time.  X3_ASYNC_REPORT=<file> writes the report."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import async_analysis_cases as AA
import async_cases as AC
import events_ref as E
import quantiles_ref as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch     # (bench.py's order: torch first, its HIP runtime serves the library too)
    return torch


@pytest.fixture(scope="module")
def x3(torch):
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def report():
    t0 = time.perf_counter()
    first = len(AC.LOG)
    yield AC.log
    AC.log("run time of tests/test_gpu_async_analysis.py: %.1f s" % (time.perf_counter() - t0))
    path = os.environ.get("X3_ASYNC_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(AC.LOG[first:]) + "\n")


@pytest.fixture(scope="module")
def cycles_per_ms(torch, report):
    return AC.calibrate_sleep(torch)


# ------------------------------------------------------------------------------------------------ A

@pytest.mark.parametrize("case", AA.CASES, ids=lambda c: c.name)
def test_behind_a_stalled_stream(x3, torch, cycles_per_ms, case):
    """the call's inputs hold a decoy when it is enqueued; the content arrives behind a stall that is proven to be still
    running when the last enqueue returns; clones taken in stream order and the originals equal the references' results"""
    AC.run_stalled(x3, torch, case, cycles_per_ms)


def test_the_events_tile_is_the_one_the_cases_are_laid_round(x3):
    ctx = x3.Context(0)
    try:
        assert ctx.get_option("events_tile_rows") == AA.EVENTS_TILE
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ B

THREADS = (("fir4", AA.TRULE_M), ("fir121", Q.TRule(peak=(500_000, 20, 1, 0))))


def test_two_threads_two_contexts_one_corpus(x3, report):
    """a context per host thread, started behind a barrier, both on ONE corpus (the header refuses a corpus call only for a
    context on another device than the build's): 25 rounds of the corpus chain each, with different taps and threshold
    rules, every output held against references computed before the threads start"""
    ROUNDS = 25
    want = [AA.corpus_chain_expect("B", sig, trule) for sig, trule in THREADS]
    for out, res in want:
        assert 3 <= res["events"][1] < AA.C_CAP
    assert want[0][1]["events"] != want[1][1]["events"] and not np.array_equal(want[0][0]["thr"], want[1][0]["thr"])
    buf, offs, lens = AA.corpus_content("B")[:3]
    owner = x3.Context(0)
    corpus = x3.Corpus(owner, buf, offs, lens, AA.c_params(x3), seg_blocks=AA.SB)
    barrier = threading.Barrier(len(THREADS))
    errors = []

    def work(k):
        ctx, bufs = None, {}
        try:
            sig, trule = THREADS[k]
            out, res = want[k]
            ctx = x3.Context(0)
            bufs = {name: ctx.alloc(n) for name, n in AA.CHAIN_OUTPUTS.items()}
            canary = {name: np.full(n, AC.CANARY, dtype=np.uint8) for name, n in AA.CHAIN_OUTPUTS.items()}
            barrier.wait()
            for rnd in range(ROUNDS):
                for name, q in bufs.items():
                    ctx.upload(q, canary[name])
                AA.corpus_chain_enqueue(x3, ctx, corpus, bufs, sig, trule)
                got = AA.corpus_chain_results(ctx)
                assert got == res, (k, rnd, got, res)
                for name, q in bufs.items():
                    a = ctx.download(q, AA.CHAIN_OUTPUTS[name])
                    assert np.array_equal(a, AA.u8(out[name])), (k, rnd, name, int(np.flatnonzero(a != AA.u8(out[name]))[0]))
        except BaseException as e:   # noqa: BLE001 -- re-raised in the main thread
            errors.append((k, e))
            barrier.abort()
        finally:
            if ctx is not None:
                for q in bufs.values():
                    ctx.free(q)
                ctx.close()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(THREADS))]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        corpus.close()
        owner.close()
    report("two threads, two contexts, one corpus: %d rounds of the corpus chain each, events found %s" % (
        ROUNDS, [w[1]["events"][1] for w in want]))
    if errors:
        raise errors[0][1]


# ------------------------------------------------------------------------------------------------ C

def _overwrite(struct, other):
    C.memmove(C.byref(struct), C.byref(other), C.sizeof(struct))


def test_host_structs_are_read_at_the_call(x3, torch, cycles_per_ms, report):
    """the content is resident and the stream stalled; x3_fir_levels_dev, x3_events_dev and x3_level_thresholds_dev are
    enqueued and the caller's x3_level_fir, x3_event_rule and x3_threshold_rule are overwritten on the host before the
    stall ends: the results are those of the structs as they were at the call (include/x3hip.h: "read at the call")"""
    rule, rule2 = AA.EV_RULE._replace(mean_sq_min=1_000_000), E.Rule(peak_min=20_000, join_bins=4, pad_bins=2, max_bins=5)
    trule, trule2 = AA.TRULE, Q.TRule(peak=(100_000, 7, 3, 11))
    lv, lv2 = AA.stream_levels("B", "fir3"), AA.stream_levels("B", "fir8")
    ev, ev2 = E.stream_events(lv, AA.N0, AA.BIN, rule), E.stream_events(lv, AA.N0, AA.BIN, rule2)
    thr, thr2 = Q.stream_thresholds(lv, AA.N0, AA.BIN, trule), Q.stream_thresholds(lv, AA.N0, AA.BIN, trule2)
    assert not np.array_equal(lv, lv2) and ev[0] != ev2[0] and thr != thr2 and 3 <= len(ev[0]) < AA.EV_CAP
    _, w_st, w_ln, w_lv = E.slots(ev[0], ev[1], AA.EV_CAP, False)
    want = {"lv": lv, "ev_st": w_st, "ev_ln": w_ln, "ev_lv": w_lv, "cnt": AA.word(len(ev[0])), "thr": AA.thr_records(thr)}
    S = torch.cuda.Stream()
    ctx = x3.Context(0, stream=S.cuda_stream)
    try:
        with torch.cuda.stream(S):
            def dev(a):
                return torch.from_numpy(AA.u8(a).copy()).to("cuda")
            d_x3, d_off = dev(AA.x3_bytes()["B"]), dev(AA.offsets("B"))
            d_so = torch.empty(8 * (AA.F0 + 1), dtype=torch.uint8, device="cuda")
            outs = {k: torch.empty(AA.u8(v).size, dtype=torch.uint8, device="cuda") for k, v in want.items()}
            d = {k: t.data_ptr() for k, t in outs.items()}
            p = x3.Params.default()
            assert ctx.sample_offsets_dev(d_x3.data_ptr(), AA.x3_len(), d_off.data_ptr(), AA.F0, d_so.data_ptr()) == 0
            tot = d_so.data_ptr() + 8 * AA.F0
            stall_ms = 0.0          # (the first pass warms the workspaces up without a stall; it proves nothing)
            for attempt in range(5):
                for t in outs.values():
                    t.fill_(AC.CANARY)
                S.synchronize()
                fir, other_fir = AA.fir_of(x3, "fir3").c_struct(), AA.fir_of(x3, "fir8").c_struct()
                r, other_r = AA.event_rule(x3, rule), AA.event_rule(x3, rule2)
                tr, other_tr = AA.threshold_rule(x3, trule), AA.threshold_rule(x3, trule2)
                if stall_ms:
                    torch.cuda._sleep(int(stall_ms * cycles_per_ms))
                behind = torch.cuda.Event()
                behind.record(S)
                assert ctx.fir_levels_dev(d_x3.data_ptr(), AA.x3_len(), d_off.data_ptr(), d_so.data_ptr(), AA.F0, p, AA.BIN,
                                          d["lv"], AA.NB, fir=fir) == 0, ctx.last_error()
                _overwrite(fir, other_fir)
                assert ctx.events_dev(d["lv"], AA.NB, AA.BIN, tot, r, d["ev_st"], d["ev_ln"], d["ev_lv"], AA.EV_CAP,
                                      d["cnt"]) == 0, ctx.last_error()
                _overwrite(r, other_r)
                assert ctx.level_thresholds_dev(d["lv"], AA.NB, AA.BIN, tot, tr, d["thr"]) == 0, ctx.last_error()
                _overwrite(tr, other_tr)
                proven = bool(stall_ms) and not behind.query()
                S.synchronize()
                if not stall_ms:
                    stall_ms = 5.0
                    continue
                report("host structs: three calls and three overwrites behind a stall of %.1f ms: %s" % (
                    stall_ms, "proven" if proven else "NOT proven"))
                if proven:
                    break
                stall_ms *= 2
            else:
                raise AssertionError("the stall was never proven: the structs were overwritten behind its end")
            assert fir.n_taps == 8 and r.max_bins == 5 and tr.peak_mul == 7          # (the overwrites took place)
            assert ctx.levels_result() == (0, 0, AA.F0, 0)
            assert ctx.events_result() == (0, len(ev[0])) and ctx.level_quantiles_result() == (0, 0, 1)
            for k, v in want.items():
                got = outs[k].cpu().numpy()
                assert np.array_equal(got, AA.u8(v)), "%s is not the result of the struct as it was at the call (byte %d)" % (
                    k, int(np.flatnonzero(got != AA.u8(v))[0]))
    finally:
        ctx.close()
