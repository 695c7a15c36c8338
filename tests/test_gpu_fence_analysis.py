"""The random-access and analysis calls under guard pages (x3-rust_amd/csrc/x3_fence.h): test_gpu_fence.py holds the codec
under X3HIP_FENCE; this module holds what came after it -- windows, ranges, the levels of every signal, the range-levels
forms, events, quantiles, thresholds, plane events and all corpus forms.  include/x3hip.h promises for every one of them
that nothing outside [d_x3, d_x3 + x3_len) is read and nothing outside the named outputs is written; a comparison of values
does not see an access a few bytes behind a buffer, an unmapped page does.

Every test is a CHILD process with X3HIP_FENCE=16, X3HIP_FENCE_FILL=165 and X3HIP_FENCE_TIGHT=1: buffers end (rounded up to
16 bytes) at the last byte of their mapping, fresh buffers are not zero, and the library's own workspaces are exactly the
bytes their carve asks for, so the last piece of a workspace ends its mapping too.  Workspaces never shrink: each child, and
each fuzz run inside it, works on a Context of its own, sized by its own small shapes.  A fault kills the child; the parent
sees the signal.

  A  the fuzz families of tools/fuzz_parity.py behind the codec's: one test per family, three runs of 50 trials
  B  tests/fence_cases.py: exact-fit buffers at the edges a random draw seldom meets, every output == its reference

Times of every child on an MI355X: profiles/fence_analysis/README.md."""
import os
import subprocess
import sys
import textwrap

import pytest

import fence_cases as FC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FAMILIES = "cxrhlitopquv"
TRIALS = 50          # per run; three runs a family
SEEDS = (11, 12, 13)


def _child(code, timeout=300, extra=None, both=False):
    """test_gpu_fence._child with the tight workspaces on top (extra: more of the environment, None takes a name out)"""
    env = dict(os.environ, **FC.ENV)
    for k, v in (extra or {}).items():
        env.pop(k, None) if v is None else env.update({k: v})
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x3-rust_amd"), HERE, os.path.join(ROOT, "tools"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-15:])
    assert r.returncode == 0, "child under the fence ended with %d:\n%s" % (r.returncode, tail)
    return (r.stdout, r.stderr) if both else r.stdout


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fuzz_family_under_the_fence(family):
    """150 trials of one family: three runs of 50 with a seed and a Context of their own, so that the workspaces of a run are
    sized by its own first trials and not by an earlier large one"""
    out = _child("""
        import fuzz_parity as FZ
        total = 0
        for seed in %r:
            c = FZ.run(seed=seed, trials=%d, families=%r, context=None)
            assert sum(c.values()) == c[%r]
            total += c[%r]
            print("run", seed, c[%r], flush=True)
        print("trials", total)
        """ % (SEEDS, TRIALS, family, family, family, family))
    assert int(out.split("trials")[1]) == len(SEEDS) * TRIALS


@pytest.mark.parametrize("group", FC.GROUPS)
def test_exact_fit_cases_under_the_fence(group):
    """every case of one group of fence_cases.py on a fresh Context: buffers of exactly the bytes the header asks for, every
    output == its reference, the result calls too; the child says how many cases it ran"""
    out = _child("""
        import x3hip, fence_cases as FC
        ctx = x3hip.Context(0)
        done = FC.run_group(x3hip, ctx, %r)
        ctx.close()
        print("cases", done)
        """ % group)
    assert int(out.split("cases")[1]) == FC.COUNTS[group]


@pytest.mark.parametrize("tight", [True, False])
def test_the_switch_makes_a_workspace_exactly_its_carve(tight):
    """X3HIP_FENCE_TIGHT: with X3HIP_FENCE_LOG every guarded allocation is written to stderr.  One levels call of a stream of
    two frames on a fresh Context: what the library allocates behind the caller's own buffers is its workspace, a few
    256-byte pieces and the eight bytes of its last one with the switch on, 4 096 bytes rounded to 256 without it"""
    out, err = _child("""
        import sys
        import x3hip, fence_cases as FC
        ctx = x3hip.Context(0)
        mine = []
        alloc = ctx.alloc
        ctx.alloc = lambda n: (mine.append(n), alloc(n))[1]
        sys.stderr.write("MARK\\n"); sys.stderr.flush()
        s = FC.stream("m2_7")
        src = FC.Source(x3hip, ctx, s)
        case = [c for c in FC.b2_stream_cases(s) if c.name == "levels_m2_7_samples_bin0"][0]
        FC.run_case(x3hip, ctx, src, case)
        src.close()
        ctx.close()
        print("mine", " ".join(str(n) for n in mine))
        """, extra={"X3HIP_FENCE_LOG": "1", "X3HIP_FENCE_TIGHT": "1" if tight else None}, both=True)
    mine = sorted(int(v) for v in out.split("mine")[1].split())
    logged = sorted(int(line.split(" + ")[1].split()[0]) for line in err.split("MARK")[1].splitlines() if line.startswith("x3_fence:"))
    for n in mine:
        logged.remove(n)
    assert logged, "the call allocated no workspace"
    if tight:
        assert any(n < 4096 and n % 256 == 8 for n in logged), logged
    else:
        assert all(n >= 4096 and n % 256 == 0 for n in logged), logged
