"""CPU: the numpy restatements of the motif kernels against the definitions -- tokens on hand-built rolls, the longest
common run against a brute-force scan, a planted transposed motif, the ranking -- and the command-line tool with --cpu."""
import json
import os
import re

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi_rolls as MR
from melo_gan_amd import motifs as M

import motif_cases as MC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REST = (0, -1, 0)


def tokens_of(events, mode=0, T=None, poke=None):
    ev = np.asarray(events, np.int64).reshape(-1, 4)
    x = MC.rolls_of([ev], T or max(1, ev.shape[0]))
    if poke is not None:
        x[0, poke, 2] = np.nan
    t, n = M.host_tokens(x, mode)
    assert (t[0, n[0]:] == M.PAD).all()
    return t[0, :n[0]].tolist()


def tok(interval, rhythm):
    return (interval + 64) | (rhythm << 7)


def test_tokens_interval_and_rhythm_of_neighbouring_notes():
    ev = [(60, 90, 32, 16), (64, 90, 32, 64), (57, 90, 32, 200), (57, 90, 32, 7)]
    assert tokens_of(ev) == [tok(4, 1), tok(-7, 3), tok(0, 5)]
    assert tokens_of(ev, mode=1) == [tok(4, 0), tok(-7, 0), tok(0, 0)]       # mode `interval`: no rhythm bits
    # the padding row is a rest: it adds time behind the last note and no token
    assert tokens_of(ev, T=9) == [tok(4, 1), tok(-7, 3), tok(0, 5)]


def test_a_rest_between_two_notes_lengthens_the_ioi_class():
    assert tokens_of([(60, 90, 16, 16), (62, 90, 16, 16)]) == [tok(2, 1)]
    assert tokens_of([(60, 90, 16, 16), (*REST, 16), (62, 90, 16, 16)]) == [tok(2, 2)]         # 32 ticks
    assert tokens_of([(60, 90, 16, 16), (*REST, 16), (*REST, 64), (62, 90, 16, 16)]) == [tok(2, 4)]       # 96 ticks


def test_a_non_finite_event_is_skipped_and_takes_no_time():
    ev = [(60, 90, 16, 16), (70, 90, 16, 256), (62, 90, 16, 16)]
    assert tokens_of(ev) == [tok(10, 1), tok(-8, 5)]
    assert tokens_of(ev, poke=1) == [tok(2, 1)]


def test_rows_with_fewer_than_two_sounding_notes_have_no_tokens():
    x = MC.rolls_of([[(*REST, 16)] * 4, [(*REST, 16), (60, 90, 16, 16), (*REST, 16)], [(60, 90, 16, 16), (61, 90, 16, 16)]], 5)
    x[0, 2] = np.inf
    t, n = M.host_tokens(x)
    assert n.tolist() == [0, 0, 1] and n.dtype == np.int32 and t.dtype == np.uint16
    assert (t[:2] == M.PAD).all() and t[2].tolist() == [tok(1, 1)] + [M.PAD] * 4


@pytest.mark.parametrize("edge", M.RHYTHM_EDGES)
def test_the_five_rhythm_boundaries(edge):
    k = M.RHYTHM_EDGES.index(edge)
    assert tokens_of([(60, 90, 16, edge - 1), (60, 90, 16, 16)]) == [tok(0, k)]
    assert tokens_of([(60, 90, 16, edge), (60, 90, 16, 16)]) == [tok(0, k + 1)]


def test_ticks_are_rounded_to_the_nearest_sixty_fourth_of_a_beat():
    # a step below the contract's floor decodes to 0.1 beat = 6 ticks; 4 beats = 256
    x = MC.rolls_of([[(60, 90, 16, 3), (60, 90, 16, 256)]], 2)
    from melo_gan_amd.gan.music_metrics import decode_rolls
    assert M.event_ticks(decode_rolls(x)).tolist() == [[6, 256]]
    assert tokens_of([(60, 90, 16, 3), (*REST, 3), (60, 90, 16, 16)]) == [tok(0, 1)]        # 6 + 6 = 12 ticks


def test_host_lcs_equals_a_brute_force_scan_with_tie_break_and_reach():
    g = np.random.default_rng(5)
    cases = 0
    for symbols in (2, 3, 4):
        for _ in range(40):
            T = 12
            qs = [g.integers(0, symbols, g.integers(0, T + 1)) for _ in range(3)]
            cs = [g.integers(0, symbols, g.integers(0, T + 1)) for _ in range(4)]
            qt, ql = MC.token_rows(qs, T)
            ct, cl = MC.token_rows(cs, T)
            packed, reach = M.host_lcs(qt, ql, ct, cl)
            L, ie, je = M.unpack(packed)
            for q, a in enumerate(qs):
                want_reach = np.zeros(T, np.int64)
                for c, b in enumerate(cs):
                    bl, bi, bj, br = MC.brute_lcs(a, b)
                    assert (L[q, c], ie[q, c], je[q, c]) == (bl, bi, bj), (a, b)
                    want_reach[:len(a)] = np.maximum(want_reach[:len(a)], br)
                    cases += 1
                assert reach[q].tolist() == want_reach.tolist()
    assert cases == 3 * 40 * 12


def test_packed_values_order_by_length_then_earlier_positions():
    p = M.pack([3, 3, 3, 2, 0], [5, 4, 4, 0, -1], [0, 9, 2, 0, -1])
    assert p[4] == 0 and p[2] > p[1] > p[0] > p[3] > p[4]
    assert [x.tolist() for x in M.unpack(p)] == [[3, 3, 3, 2, 0], [5, 4, 4, 0, -1], [0, 9, 2, 0, -1]]


def test_a_run_does_not_continue_from_the_end_of_b_into_its_start():
    a = [1, 2, 3, 4]
    qt, ql = MC.token_rows([a], 6)
    ct, cl = MC.token_rows([[3, 4, 9, 1, 2]], 6)        # 1 2 | 3 4 only across b's end
    L, ie, je = M.unpack(M.host_lcs(qt, ql, ct, cl)[0])
    assert (L[0, 0], ie[0, 0], je[0, 0]) == (2, 1, 4)
    # and tokens behind a row's length are not matched, whatever they hold
    ct[0, 5] = 3
    qt[0, 4] = 9
    packed, reach = M.host_lcs(qt, ql, ct, cl)
    assert M.unpack(packed)[0][0, 0] == 2 and reach[0].tolist() == [1, 2, 1, 2, 0, 0]


def test_pairs_of_equal_groups_are_skipped():
    qt, ql = MC.token_rows([[1, 2, 3], [1, 2, 3]], 4)
    ct, cl = MC.token_rows([[1, 2, 3], [2, 3], [7]], 4)
    packed, reach = M.host_lcs(qt, ql, ct, cl, np.array([0, 5], np.int32), np.array([0, 1, 5], np.int32))
    L = M.unpack(packed)[0]
    assert L.tolist() == [[0, 2, 0], [3, 2, 0]]
    assert reach.tolist() == [[0, 1, 2, 0], [1, 2, 3, 0]]
    # a query all of whose pairs are skipped
    packed, reach = M.host_lcs(qt[:1], ql[:1], ct, cl, np.array([3], np.int32), np.array([3, 3, 3], np.int32))
    assert not packed.any() and not reach.any()


def test_host_rank_ties_go_to_the_lower_row_and_the_tail_is_empty():
    p = np.array([[5, 9, 9, 0, 5], [0, 0, 0, 0, 0]], np.int64)
    vals, idx = M.host_rank(p, 3)
    assert vals.tolist() == [[9, 9, 5], [0, 0, 0]] and idx.tolist() == [[1, 2, 0], [0, 1, 2]]
    vals, idx = M.host_rank(p, 7)
    assert vals[0].tolist() == [9, 9, 5, 5, 0, 0, 0] and idx[0].tolist() == [1, 2, 0, 4, 3, -1, -1]
    assert idx.dtype == np.int32 and vals.dtype == np.int64


def test_copied_share_covers_the_runs_that_reach_min_len():
    reach = np.array([1, 2, 3, 0, 1, 2, 1, 0], np.int32)
    assert M.copied_share(reach, 8, 3) == 3 / 8
    assert M.copied_share(reach, 8, 2) == 5 / 8          # 0..2 by the 3 (the 2 inside it adds nothing), 4..5
    assert M.copied_share(reach, 8, 4) == 0.0 and M.copied_share(reach, 0, 1) == 0.0


@pytest.fixture(scope="module")
def planted():
    """Random-walk rows; 16 notes of corpus row 1 (15 tokens, from note 20) stand in query row 0 from note 50, three
    semitones higher."""
    g = np.random.default_rng(3)
    T = 96
    corpus = [MC.walk_events(g, T, rests=0.0) for _ in range(4)]
    query = [MC.walk_events(g, T, rests=0.0) for _ in range(3)]
    query[0][50:66] = corpus[1][20:36]
    query[0][50:66, 0] += 3
    q, c = MC.rolls_of(query, T), MC.rolls_of(corpus, T)
    return q, c, M.host_match(q, c, top=2)


def test_a_planted_motif_is_found_transposed_and_shifted(planted):
    q, c, m = planted
    L, ie, je = M.unpack(m.vals)
    assert m.idx[0, 0] == 1 and L[0, 0] >= 15
    i0, j0 = ie[0, 0] - L[0, 0] + 1, je[0, 0] - L[0, 0] + 1
    assert i0 <= 50 and ie[0, 0] >= 64 and i0 - j0 == 30           # tokens 50..64 against 20..34
    rows = M.describe(m, M.RollSet(q, sources=["q%d" % i for i in range(3)]), M.RollSet(c, sources=["c%d" % i for i in range(4)]), 8)
    top = rows[0]["matches"][0]
    assert top["corpus_row"] == 1 and top["source"] == "c1" and top["length"] == L[0, 0] and top["transposition"] == 3
    assert top["query_event"] == i0 and top["corpus_event"] == j0 and top["distinct_tokens"] >= 8
    assert rows[0]["copied_share"] >= 15 / rows[0]["tokens"] and rows[0]["tokens"] == 95
    # the unrelated rows: chance runs stay below --min-len 8
    for r in rows[1:]:
        assert r["copied_share"] == 0.0 and r["matches"] == [] and 1 <= r["longest"] < 8


def test_the_signature_table_covers_the_motif_entry_points():
    from melo_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "melo_gan_hip.h")).read()
    for name, nargs in (("mg_motif_tokens", 7), ("mg_motif_lcs", 12), ("mg_motif_rank", 7)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs == decl.group(1).count(",") + 1


# ---- the tool, --cpu ----

@pytest.fixture(scope="module")
def midi_files(tmp_path_factory):
    return MC.write_midi_cases(str(tmp_path_factory.mktemp("motif_midi")))


def run_tool(argv, capsys):
    rc = M.main(argv)
    out = capsys.readouterr()
    return rc, out.out, out.err


def test_cli_finds_the_shared_phrase_in_another_key(midi_files, tmp_path, capsys):
    out = str(tmp_path / "motifs.json")
    rc, said, err = run_tool([midi_files["b"], midi_files["c"], "--corpus", midi_files["a"], "--cpu", "--out", out], capsys)
    assert rc == 0, err
    lines = [ln for ln in said.splitlines() if ln.startswith("motifs: ")]
    assert len(lines) == 2 and midi_files["b"] in lines[0] and midi_files["c"] in lines[1]      # one line per query file
    rep = json.load(open(out))
    assert rep["tokens"] == "interval+rhythm" and rep["min_len"] == 8 and rep["top"] == 3 and rep["device"] is False
    assert rep["corpus"] == {"rows": 1, "files": 1} and len(rep["rows"]) == 2
    b, c = rep["rows"]
    n = midi_files["phrase_notes"]
    assert b["source"] == midi_files["b"] + "@0" and b["tokens"] == 11 + n + 9 - 1
    assert set(b) == {"row", "source", "tokens", "longest", "matches", "copied_share"}
    (hit,) = b["matches"]
    assert set(hit) == {"corpus_row", "source", "length", "query_event", "corpus_event", "transposition", "distinct_tokens"}
    assert hit["corpus_row"] == 0 and hit["source"] == midi_files["a"] + "@0" and hit["transposition"] == MC.PHRASE_SHIFT
    assert hit["length"] == b["longest"] == n - 1 and hit["distinct_tokens"] >= 10
    assert hit["query_event"] == 11 and hit["corpus_event"] == 6         # the phrase's first note in b and in a
    assert b["copied_share"] == hit["length"] / b["tokens"]
    assert c["matches"] == [] and c["copied_share"] == 0.0 and c["longest"] < 8
    s = rep["summary"]
    assert s["rows"] == 2 and s["max_longest"] == hit["length"] and s["mean_longest"] == (b["longest"] + c["longest"]) / 2
    assert list(s["share_longest_at_least"]) == ["4", "8", "12", "16", "24", "32"]
    assert s["share_longest_at_least"]["16"] == 0.5 and s["share_longest_at_least"]["24"] == 0.0
    assert s["mean_copied_share"] == b["copied_share"] / 2


def test_cli_interval_mode_and_min_len(midi_files, tmp_path, capsys):
    out = str(tmp_path / "m.json")
    rc, _, err = run_tool([midi_files["b"], "--corpus", midi_files["a"], "--cpu", "--out", out, "--tokens", "interval",
                           "--min-len", "40", "--top", "1"], capsys)
    assert rc == 0, err
    rep = json.load(open(out))
    row = rep["rows"][0]
    assert rep["tokens"] == "interval" and row["matches"] == [] and row["copied_share"] == 0.0
    assert row["longest"] >= midi_files["phrase_notes"] - 1


def test_cli_self_reports_each_pair_once(midi_files, tmp_path, capsys):
    out = str(tmp_path / "self.json")
    folder = os.path.dirname(midi_files["a"])
    rc, said, err = run_tool(["--corpus", folder, "--self", "--cpu", "--out", out], capsys)
    assert rc == 0, err
    rep = json.load(open(out))
    assert rep["self"] is True and [r["source"] for r in rep["rows"]] == [midi_files[k] + "@0" for k in "abc"]
    a, b, c = rep["rows"]
    assert [m["corpus_row"] for m in a["matches"]] == [1] and [m["corpus_row"] for m in b["matches"]] == [0]
    assert a["matches"][0]["transposition"] == -MC.PHRASE_SHIFT and b["matches"][0]["transposition"] == MC.PHRASE_SHIFT
    assert c["matches"] == []
    (pair,) = rep["pairs"]
    assert (pair["row"], pair["corpus_row"]) == (0, 1) and pair["length"] == a["longest"]
    assert "1 pairs" in said
    # windows of one file are one group: with a hop below the window, a file's overlapping windows do not match each other
    rc, _, err = run_tool(["--corpus", midi_files["a"], "--self", "--cpu", "--out", out, "--max-notes", "16", "--hop", "4"], capsys)
    assert rc == 0, err
    rep = json.load(open(out))
    assert len(rep["rows"]) > 2 and rep["pairs"] == [] and all(r["longest"] == 0 for r in rep["rows"])


def test_cli_baseline_and_npy_and_split_inputs(midi_files, tmp_path, capsys):
    from melo_gan_amd import midi_import
    split = str(tmp_path / "split")
    assert midi_import.main([midi_files["a"], midi_files["c"], "--out", split, "--max-notes", "64", "--cpu"]) == 0
    rolls = str(tmp_path / "rolls.npy")
    p = MR.plan_files([midi_files["b"]], 48, 48, 8)
    np.save(rolls, MR.host_roll_encode(p.events, p.win_start, p.win_len, p.T)[0])
    out = str(tmp_path / "base.json")
    rc, said, err = run_tool([rolls, "--corpus", split, "--baseline", midi_files["c"], "--cpu", "--out", out], capsys)
    assert rc == 0, err
    rep = json.load(open(out))
    assert rep["max_notes"] == 512 and rep["corpus"] == {"rows": 2, "files": 2}        # the baseline's MIDI windows are the longest rows
    row = rep["rows"][0]
    assert row["source"] == rolls + "#0" and row["matches"][0]["source"] == midi_files["a"] + "@0"
    assert row["matches"][0]["transposition"] == MC.PHRASE_SHIFT
    base = rep["baseline"]
    assert set(base) == {"rows", "summary"} and set(base["summary"]) == set(rep["summary"])
    # c.mid against a corpus that holds c.mid: the whole row is shared
    held = base["rows"][0]
    assert held["copied_share"] == 1.0 and held["matches"][0]["corpus_row"] == 1 and held["matches"][0]["transposition"] == 0
    assert base["summary"]["mean_copied_share"] == 1.0 and "against the baseline's" in said


@pytest.mark.parametrize("case", ["missing", "empty", "top0", "self+query", "no-corpus", "tokens", "device"])
def test_cli_error_paths_end_with_status_2_and_the_error_line(case, midi_files, tmp_path, capsys):
    a, empty = midi_files["a"], str(tmp_path / "empty")
    os.makedirs(empty, exist_ok=True)
    argv = {"missing": [str(tmp_path / "nothing.mid"), "--corpus", a, "--cpu"],
            "empty": [a, "--corpus", empty, "--cpu"],
            "top0": [a, "--corpus", a, "--cpu", "--top", "0"],
            "self+query": [a, "--corpus", a, "--cpu", "--self"],
            "no-corpus": [a, "--cpu"],
            "tokens": [a, "--corpus", a, "--cpu", "--tokens", "chords"],
            "device": [a, "--corpus", a]}[case]
    if case == "device":
        import torch
        if torch.cuda.is_available():
            argv = argv + ["--batch", "0"]
    rc, said, err = run_tool(argv + ["--out", str(tmp_path / "never.json")], capsys)
    assert rc == 2 and err.startswith("motifs: error: ") and len(err.splitlines()) == 1 and said == ""
    assert not os.path.exists(str(tmp_path / "never.json"))
