"""The preconditions of the stalled-stream cases (async_cases.py), from the CPU oracle alone: a case can only catch a call
that reads its inputs early if the decoy A and the content B give different answers in everything the case compares, and
it may only run on a shared GPU if A is valid, in bounds everywhere, for the shapes B's calls use."""
import numpy as np
import pytest

import async_cases as AC


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.name)
def test_decoy_and_content_differ_in_every_compared_output(case):
    AC.check_pair_differs(case)


def test_case_names_are_unique():
    names = [c.name for c in AC.CASES]
    assert len(set(names)) == len(names)


def test_the_damaged_stream_fails_where_the_cases_say():
    s, st = AC.damaged_b()
    clean, offs, _ = AC.encoded("B")
    assert s.size == clean.size and np.flatnonzero(st).tolist() == [9, 30]
    assert st[9] == AC.ERR_PAYLOAD_CRC and st[30] not in (0, AC.ERR_PAYLOAD_CRC)
    # the walk of the whole stream stops at the CRC failure, with the samples of the nine frames in front of it
    rc, w, fok, ferr = AC.O.decode_stream(s, AC.oparams(), wav_cap=AC.N0)
    assert (rc, w.size, fok) == (AC.ERR_PAYLOAD_CRC, 9 * AC.SPF, 9)
    # frame 30 alone: valid CRCs, a payload that does not decode
    o = int(offs[30])
    rc, w, fok, ferr = AC.O.decode_stream(s[o:int(offs[31])], AC.oparams(), wav_cap=AC.SPF)
    assert (rc, fok, ferr) == (0, 0, 1)


def test_loud_frames_are_beyond_the_wave_encoders_image():
    """payloads of more than 9 728 bytes take the dense pass behind the encode kernel (include/x3hip.h, "Content")"""
    for which, loud in (("A", (7, 31)), ("B", (5, 6, 20))):
        offs = AC.encoded(which)[1].astype(np.int64)
        sizes = np.diff(offs) - 20
        assert sorted(np.flatnonzero(sizes > 9728).tolist()) == list(loud)
