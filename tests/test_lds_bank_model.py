"""Non-GPU: the LDS bank model (tools/lds_bank_model.py) on the decode GEMMs' cross-wave reduction buffer.

The model encodes the per-instruction lane groups and bank functions of the CDNA4 LDS and returns the array cycles of one
wave-instruction from its lane -> byte-address map.  Held here: the linear reduction-buffer rows are an 8-way store conflict
(64 cycles per ds_write_b128), the swizzled layout of kernels_skinny.hip (chunk c of row b at slot c ^ (b & 7)) is conflict-free
on the store AND on the load for every workgroup form, writer and reader address the same bytes, and nothing else in the
decode chain is worse than 2-way."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

FORMS = [(nw, rb) for nw in (4, 8) for rb in (1, 2, 3, 4)] + [(16, 1)]


def test_the_model_reproduces_the_textbook_cases():
    assert M.cycles("ds_read_b32", lambda l: 4 * l) == 2 and M.ways("ds_read_b32", lambda l: 4 * l) == 1
    assert M.ways("ds_read_b32", lambda l: 128 * l) == 32                        # a column of a 32-float row-major tile
    assert M.ways("ds_read_b32", lambda l: 132 * l) == 1                         # ... padded to 33 floats
    assert M.ways("ds_read_b32", lambda l: 0) == 1                               # identical addresses broadcast
    assert M.ways("ds_read_b32", lambda l: 128 * (l >> 5)) == 1                  # lanes l and l + 32 are different groups
    assert M.ways("ds_read_b32", lambda l: 128 * ((l >> 4) & 1)) == 2            # lanes l and l + 16 are not
    assert M.cycles("ds_read_b64", lambda l: 8 * l) == 2 and M.cycles("ds_read_b128", lambda l: 16 * l) == 4
    assert M.cycles("ds_write_b64", lambda l: 8 * l) == 4 and M.cycles("ds_write_b128", lambda l: 16 * l) == 8
    assert M.ways("ds_read_b128", lambda l: 256 * l) == 16                       # 256-byte rows read by ds_read_b128
    assert M.ways("ds_write_b128", lambda l: 128 * l) == 8
    assert M.cycles("ds_write_b32", lambda l: 0 if l == 0 else None) == 1        # inactive lanes take no part
    groups = M.INSTRUCTIONS["ds_read_b128"][0]
    assert sorted(l for g in groups for l in g) == list(range(64)) and all(len(g) == 16 for g in groups)


@pytest.mark.parametrize("nw,rb", FORMS)
def test_linear_rows_are_an_8_way_store_conflict(nw, rb):
    for wave in range(nw):
        for g in range(rb):
            for q in range(4):
                m = M.red_write(wave, g, q, rb, swizzle=False)
                assert M.ways("ds_write_b128", m) == 8 and M.cycles("ds_write_b128", m) == 64
                assert M.conflict_cycles("ds_write_b128", m) == 56


@pytest.mark.parametrize("nw,rb", FORMS)
def test_swizzled_store_and_load_are_conflict_free(nw, rb):
    for wave in range(nw):
        for g in range(rb):
            for q in range(4):
                m = M.red_write(wave, g, q, rb, swizzle=True)
                assert M.group_cycles("ds_write_b128", m) == [1] * 8, (wave, g, q)
    for rpb in (32, 20):
        for wave in range(nw):                      # waves past the fourth hold no reader thread
            for src in range(nw):
                for g in range(rb):
                    c = M.group_cycles("ds_read_b128", M.red_read(wave, src, g, rb, True, rpb))
                    assert c == ([1] * 4 if wave < 4 else [0] * 4), (rpb, wave, src, g, c)


@pytest.mark.parametrize("swizzle", [False, True])
@pytest.mark.parametrize("nw,rb", [(4, 1), (8, 3)])
def test_reader_finds_what_the_writer_stored(nw, rb, swizzle):
    """Cell (b, n) of wave w's tile of row group g: written by lane (hi, b) in store q with n = 8q + 4hi + j, read by thread
    tid = 8b + n / 4 - both maps must name the same byte, and no two cells may share one."""
    where = {}
    for w in range(nw):
        for g in range(rb):
            for q in range(4):
                m = M.red_write(w, g, q, rb, swizzle)
                for lane in range(64):
                    where[(w, g, lane & 31, 2 * q + (lane >> 5))] = m(lane)
    assert len(set(where.values())) == len(where) == nw * rb * 256
    assert max(where.values()) + 16 <= nw * rb * 4096
    for w in range(nw):
        for g in range(rb):
            for wave in range(4):
                m = M.red_read(wave, w, g, rb, swizzle)
                for lane in range(64):
                    tid = wave * 64 + lane
                    assert m(lane) == where[(w, g, tid >> 3, tid & 7)]


def test_padded_rows_would_be_two_way_on_the_load():
    assert M.ways("ds_write_b128", M.red_write_padded(0, 0, 1, 1)) == 1
    assert max(M.ways("ds_read_b128", M.red_read_padded(wave, 0, 0, 1)) for wave in range(4)) == 2


def test_nothing_else_in_the_decode_chain_is_worse_than_two_way():
    rows = M.decode_chain_table()
    assert len(rows) >= 20
    for kern, access, instr, ways, cyc, conflict in rows:
        if "linear rows" in access and instr == "ds_write_b128":
            assert ways == 8
        else:
            assert ways <= 2, (kern, access, instr, ways)


def test_committed_table_is_the_models_output(capsys):
    M.main()
    out = capsys.readouterr().out.strip().splitlines()
    with open(os.path.join(ROOT, "profiles", "lds_bank_model_decode_chain.md")) as f:
        have = [l.rstrip("\n") for l in f if l.startswith("|")]
    assert have == out
