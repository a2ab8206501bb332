"""CPU: the numpy wire stream (tests/wire_stream_reference.py) against the whole-recording sum of tests/ingest_reference.py.

Fed in pieces the stream equals `emulate_f32` of the whole recording bit for bit - both are plain float32 sums with the same
operands in the same order, so there is no tolerance - K(F) equals a count over tap indices, and the case list catches the three
bugs a stateful resampler invites: each is planted into the reference and must make it fail."""
import numpy as np
import pytest

import wire_stream_reference as ws

_cache = {}


def _case(case):
    """(raw, the whole recording's result), computed once per case."""
    if case not in _cache:
        rate, fmt, ch, pick, frames = case
        raw = ws.recording(rate, fmt, ch, frames)
        _cache[case] = (raw, ws.offline(rate, raw, fmt, ch, pick))
    return _cache[case]


def _cuttings(case):
    rate, fmt, ch, _, frames = case
    n = frames * ws.sample_bytes(fmt) * ch
    return [ws.fixed_cuts(rate, ch, fmt, n)] + [ws.random_cuts(n, seed) for seed in (1, 2, 3)]


def _equal(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}ch-pick{c[3]}")
def test_pieces_equal_the_whole(case):
    rate, fmt, ch, pick, frames = case
    raw, want = _case(case)
    assert len(want) == ws.final(rate, frames, True)
    for cuts in _cuttings(case):
        got = ws.feed(ws.Stream(rate, ch, fmt, pick), raw, cuts)
        assert _equal(got, want), cuts
    # without finish: the first K(F) samples, and the bytes of the cut-off frame stay pending
    s = ws.Stream(rate, ch, fmt, pick)
    extra = b"\x01" if ws.sample_bytes(fmt) * ch > 1 else b""          # one byte is a whole frame of mono G.711 / u8
    cuts = _cuttings(case)[1]
    got = ws.feed(s, raw + extra, cuts[:-1] + [cuts[-1] + len(extra)], finish=False)
    assert _equal(got, want[:ws.final(rate, frames)]) and s.pending == extra


@pytest.mark.parametrize("rate", sorted({c[0] for c in ws.CASES}))
def test_final_count_is_the_brute_force_count(rate):
    for F in range(601):
        assert ws.final(rate, F) == ws.final_brute(rate, F), F
    assert ws.final(rate, 600, True) == -(-600 * ws.plan(rate)[0] // ws.plan(rate)[1])


def test_rates():
    assert all(ws.stream_rate(r) for r in ws.ref.RATES + (16000,))
    assert ws.plan(192000)[3] == 240 and ws.plan(8000)[3] == 20 and ws.plan(16000)[3] == 0
    assert not ws.stream_rate(384000) and not ws.stream_rate(16000 * 1024) and not ws.stream_rate(0)
    assert [ws.final(16000, F) for F in (0, 1, 513)] == [0, 1, 513]


def test_the_fixed_cuts_of_44100_end_a_piece_where_the_oldest_history_frame_meets_a_real_tap():
    assert [ws.oldest_frame_slack(c[0]) for c in ws.CASES] == [0, 0, 0, 0, 20, 0, 0, 0]
    rate, fmt, ch, _, frames = ws.CASES[4]
    up, down, half, H = ws.plan(rate)
    cuts = ws.fixed_cuts(rate, ch, fmt, frames * 6)
    assert len(cuts) == 8 and sum(cuts[:7]) % 6 == 0
    F = sum(cuts[:7]) // 6
    k = ws.final(rate, F)
    t = k * down + half - (F - H) * up                      # the tap output K(F) applies to frame F - H
    assert F > 3 * H + 1 and 2 * half - 20 <= t <= 2 * half and abs(ws.ref.design(rate)[t]) > 1e-6
    assert all(ws.exposing_cut(c[0], 100) is None for c in ws.CASES if c[0] != 44100)


@pytest.mark.parametrize("bug", ({"drop_history": True}, {"short_history": 1}, {"k_shift": 1}, {"k_shift": -1}),
                         ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_the_case_list_catches_planted_bugs(bug):
    """The mutated stream must fail under the fixed cuttings.  A dropped history and a late K show in every case that has a
    history / in every case.  The two edge bugs - the history one frame short, an output released one frame early - move ONE
    operand, which meets a tap of the filter's outermost row.  Where that tap is h[0] = h[2 half], about 1e-18 (the sinc's zero, in
    floating point), the lost product rounds away: for the early output always so with up == 1, and at 8000 where the first
    non-final output has phase 0; for the short history wherever up divides 2 half, which is every case but 44100.  There the
    fixed cuts end a piece on an exposing cut (wire_stream_reference.exposing_cut), and that case must catch the short history;
    the early output must be caught at 44100 and 11025."""
    edge = bug.get("short_history") or bug.get("k_shift") == 1
    caught = {}
    for case in ws.CASES:
        rate, fmt, ch, pick, frames = case
        if rate == 16000 and "k_shift" not in bug:
            continue                       # no filter: there is no history to lose
        raw, want = _case(case)
        got = ws.feed(ws.Stream(rate, ch, fmt, pick, **bug), raw, _cuttings(case)[0], finish=bug.get("k_shift") != -1)
        caught[case] = not _equal(got, want if bug.get("k_shift") != -1 else want[:ws.final(rate, frames)])
    if bug.get("short_history"):
        assert caught[ws.CASES[4]], caught
    elif edge:
        assert caught[ws.CASES[4]] and caught[ws.CASES[5]], caught
    else:
        assert all(caught.values()), caught
