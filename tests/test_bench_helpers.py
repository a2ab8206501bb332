"""CPU: bench.py's token-agreement report (`output_check.vs_f32_parity_tokens`) on the committed f32 reference tokens and margins
(profiles/bench_tokens_f32.npy, _margins.npy, _runner_up.npy): identical tokens -> 32 / 32; a row that takes the f32 runner-up at a
position is reported with the f32 engine's own margin there and `took_ref_runner_up`; a row that takes some third token is not."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_token_agreement_reports_margins_at_divergences():
    b = _bench()
    ref = np.load(os.path.join(ROOT, "profiles", "bench_tokens_f32.npy"))
    mg = np.load(os.path.join(ROOT, "profiles", "bench_tokens_f32_margins.npy"))
    ru = np.load(os.path.join(ROOT, "profiles", "bench_tokens_f32_runner_up.npy"))
    assert ref.shape == mg.shape == ru.shape == (32, 128) and (mg > 0).all()        # the f32 tokens ARE the f32 argmax everywhere
    same = b.token_agreement(ref.copy(), "bench_tokens_f32.npy", "large-v3", "noise")
    assert same["rows_identical"] == 32 and same["equal_prefix_fraction"] == 1.0 and same["divergences"] == []
    mine = ref.copy()
    mine[3, 2:] = 7                      # leaves at position 2 ...
    mine[3, 2] = ru[3, 2]                # ... by taking the f32 runner-up
    mine[9, 40:] = 11                    # leaves at position 40 with a third token
    assert ru[9, 40] != 11
    out = b.token_agreement(mine, "bench_tokens_f32.npy", "large-v3", "noise")
    assert out["rows_identical"] == 30 and out["first_divergence_per_row"][3] == 2 and out["first_divergence_per_row"][9] == 40
    d = {x["row"]: x for x in out["divergences"]}
    assert set(d) == {3, 9}
    assert d[3]["took_ref_runner_up"] and abs(d[3]["ref_engine_top2_margin"] - float(mg[3, 2])) < 1e-4
    assert not d[9]["took_ref_runner_up"] and abs(d[9]["ref_engine_top2_margin"] - float(mg[9, 40])) < 1e-4
    assert abs(out["largest_ref_margin_at_a_divergence"] - max(float(mg[3, 2]), float(mg[9, 40]))) < 1e-4
    # another workload (other model / clip set) has no committed reference: no claim is made
    assert b.token_agreement(mine, "bench_tokens_f32.npy", "small", "noise") is None
    assert b.token_agreement(mine, "bench_tokens_f32.npy", "large-v3", "tonal") is None


def test_dump_outputs_writes_float64_and_a_fixed_sample_under_the_limit(tmp_path):
    b = _bench()
    toks = np.arange(64 * 16, dtype=np.int32).reshape(64, 16)
    w = b.dump_outputs(str(tmp_path / "a"), {"tokens": toks})
    got = np.load(tmp_path / "a" / "tokens.npy")
    assert got.dtype == np.float64 and np.array_equal(got, toks) and w == {"tokens": {"shape": [64, 16], "rows_of": 64}}
    # over the limit: a seeded subset of whole rows, identical from run to run
    lim = 10 * 16 * 8
    for d in ("b", "c"):
        b.dump_outputs(str(tmp_path / d), {"tokens": toks}, limit=lim)
    x, y = np.load(tmp_path / "b" / "tokens.npy"), np.load(tmp_path / "c" / "tokens.npy")
    assert x.shape == (10, 16) and x.nbytes <= lim and np.array_equal(x, y)
    rows = x[:, 0].astype(np.int64) // 16
    assert (np.diff(rows) > 0).all() and np.array_equal(x, toks[rows])


def test_seeded_weights_equal_the_serial_generator():
    """bench.py generates the synthetic weights on a few threads: same names, same order, same bits as synth.iter_weights."""
    import sys
    sys.path.insert(0, ROOT)
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import PRESETS
    b = _bench()
    dims = PRESETS["tiny"]
    got = list(b.seeded_weights(dims, workers=4, ahead=3))
    want = list(synth.iter_weights(dims))
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, x), (_, y) in zip(got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), n


def test_full_only_options_are_refused_without_full():
    """A plain run measures the headline value only: options that belong to the --full measurements fail at once (before any GPU
    work) instead of being ignored."""
    import subprocess
    import sys
    for extra in (["--write-crc"], ["--dump-tokens", "t.npy"], ["--cpu-full"], ["--more-in-flight"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "add --full" in r.stderr, (extra, r.returncode, r.stderr[-500:])
