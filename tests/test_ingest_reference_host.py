"""CPU: the float64 reference of the device file ingest (tests/ingest_reference.py) is scipy.signal.resample_poly, its float32
emulation stays under half of the derived bound on every case of the table, and the bound catches three planted bugs."""
import numpy as np
import pytest

import ingest_reference as R


@pytest.mark.parametrize("rate", R.RATES)
def test_reference_is_resample_poly(rate):
    from scipy.signal import resample_poly
    up, down = R.ratio(rate)[:2]
    for n in (1, 7, 333, 700):
        x = np.random.default_rng([rate, n]).standard_normal((n, 1))
        y, _, _ = R.direct(rate, x)
        want = resample_poly(x[:, 0], up, down)
        assert y.shape == want.shape == (R.n_out(rate, n),)
        assert np.abs(y - want).max() <= 1e-12, (rate, n, np.abs(y - want).max())


def test_case_table_covers_rates_formats_channels():
    assert {c[0] for c in R.CASES} == set(R.RATES)
    assert {c[1] for c in R.CASES} == set(range(6))
    assert {c[2] for c in R.CASES} == {1, 2, 6}
    for rate, _, _ in R.CASES + R.EXTREME_CASES:
        assert R.accepted(rate) and R.span(rate, R.tile_for(rate)) <= R.SPAN_MAX and R.tile_for(rate) >= 1


@pytest.mark.parametrize("case", R.CASES + R.EXTREME_CASES, ids=lambda c: "r%d-f%d-c%d" % c)
def test_float32_emulation_stays_under_half_the_bound(case):
    rate, fmt, ch = case
    worst = 0.0
    for n in R.lengths(rate):
        raw, y, S, T = R.cached_case(rate, fmt, ch, n)
        err = np.abs(R.emulate_f32(rate, raw, fmt, ch).astype(np.float64) - y)
        b = R.bound(S, T, ch)
        assert np.all(err[b == 0] == 0)
        worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    print(f"ingest emulation {case}: worst error / bound {worst:.3f}")
    assert worst <= 0.5, worst


def _ratios(case, planted):
    """The worst |planted - y| / bound over the lengths of a case."""
    rate, fmt, ch = case
    worst = 0.0
    for n in R.lengths(rate):
        raw, y, S, T = R.cached_case(rate, fmt, ch, n)
        got = planted(rate, R.channels_f64(raw, fmt, ch), y)
        b = R.bound(S, T, ch)
        err = np.abs(got - y)
        if np.any(b > 0):
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


def _tap_off_by_one(rate, x, y):
    return R.direct(rate, x, tap_shift=1)[0]


def _lost_halo(rate, x, y):
    """The first input of every 64th output is dropped."""
    up, down, _, half, _ = R.ratio(rate)
    out = y.copy()
    h, mono = R.design(rate), x.mean(axis=1)
    for k in range(0, len(y), 64):
        i = max(-((half - k * down) // up), 0)
        t = k * down + half - i * up
        if i < len(x) and 0 <= t <= 2 * half:
            out[k] -= mono[i] * h[t]
    return out


def _n_out_floored(rate, x, y):
    up, down = R.ratio(rate)[:2]
    out = y.copy()
    out[len(x) * up // down:] = 0.0   # the outputs a floored length never writes
    return out


@pytest.mark.parametrize("planted", (_tap_off_by_one, _lost_halo, _n_out_floored), ids=lambda f: f.__name__.strip("_"))
def test_bound_catches_planted_bug(planted):
    worst = {c: _ratios(c, planted) for c in R.CASES[::3]}
    print(f"ingest planted {planted.__name__}: error / bound per case {worst}")
    assert max(worst.values()) > 10.0, worst
