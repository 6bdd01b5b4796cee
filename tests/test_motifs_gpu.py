"""GPU: mg_motif_tokens, mg_motif_lcs and mg_motif_rank against their numpy restatements, exact integer equality throughout,
inside poisoned output buffers; Motifs.match in two batch sizes; the tool on the device against --cpu; bad arguments."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import motifs as M  # noqa: E402
from melo_gan_amd import ops  # noqa: E402

import motif_cases as MC  # noqa: E402

REST = (0, -1, 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def token_case(T):
    """N = 5 rows of T positions: a melody with rests and invalid events; all rests; all invalid; notes only on both sides
    of a wave and of a chunk boundary; a melody without rests."""
    g = np.random.default_rng(T)
    rest_row = np.array([(*REST, 16)] * T)
    edge = rest_row.copy()
    for t in (63, 64, 255, 256):
        if t < T:
            edge[t] = (60 + t % 7, 90, 16, 24)
    x = MC.rolls_of([MC.walk_events(g, T, rests=0.3), rest_row, rest_row, edge, MC.walk_events(g, T)], T)
    x[0, g.random(T) < 0.1, g.integers(0, 4)] = np.nan
    x[2, :, 1] = np.inf
    return x


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 256, 257, 600])
def test_motif_tokens_equal_the_host_padding_included(T):
    x = token_case(T)
    for mode in (ops.MOTIF_INTERVAL_RHYTHM, ops.MOTIF_INTERVAL):
        want_t, want_n = M.host_tokens(x, mode)
        tokens = torch.full((5, T), 7, dtype=torch.uint16, device="cuda")
        lengths = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        ops.motif_tokens(dev(x), mode, tokens, lengths)
        torch.cuda.synchronize()
        assert lengths.cpu().numpy().tolist() == want_n.tolist()
        assert (tokens.cpu().numpy() == want_t).all()
    assert want_n[1] == 0 and want_n[2] == 0 and want_n[3] == max(0, sum(t < T for t in (63, 64, 255, 256)) - 1)
    if T >= 63:
        assert want_n[0] > 0 and want_n[4] == T - 1


def device_lcs(qt, ql, ct, cl, qg=None, cg=None, graph=False):
    Nq, T, Nc = qt.shape[0], qt.shape[1], ct.shape[0]
    packed = torch.full((Nq, Nc), -1, dtype=torch.int64, device="cuda")
    reach = torch.full((Nq, T), 77, dtype=torch.int32, device="cuda")
    a = [dev(v) for v in (qt, ql, ct, cl)] + [None if qg is None else dev(qg), None if cg is None else dev(cg)]
    launch = lambda: ops.motif_lcs(*a, packed, reach)  # noqa: E731
    launch()
    if graph:
        torch.cuda.synchronize()
        packed.fill_(-1)
        reach.fill_(77)
        with torch.cuda.stream(torch.cuda.Stream()):
            g = ops.Graph.capture(launch)
            g.launch()
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return packed.cpu().numpy(), reach.cpu().numpy()


LCS_T = 160
LCS_LENGTHS = (0, 1, 63, 64, 65, 129, LCS_T - 1)


@pytest.fixture(scope="module")
def lcs_case():
    """5 x 7 token rows of T = 160 and the host's answer, computed once: (rows, {groups: (packed, reach)})."""
    g = np.random.default_rng(160)
    wide = lambda n: g.integers(10, 500, n)  # noqa: E731
    q2, x, y = wide(120), wide(30), wide(25)
    qs = [g.integers(0, 2, LCS_T - 1),             # two symbols: ties everywhere
          np.full(100, 5),                         # all equal
          q2,                                      # matches c5 at the very start and at the very end of both
          np.concatenate([x, y]),                  # c4 holds y at its start and x at its end: no run across the wrap
          np.array([1])]
    cs = [np.zeros(0, np.int64), np.array([1]), g.integers(0, 2, 63), np.full(64, 5), np.concatenate([y, wide(10), x]),
          np.concatenate([q2[:10], g.integers(600, 700, 107), q2[-12:]]), g.integers(0, 2, LCS_T - 1)]
    assert tuple(len(c) for c in cs) == LCS_LENGTHS
    qt, ql = MC.token_rows(qs, LCS_T)
    ct, cl = MC.token_rows(cs, LCS_T)
    groups = {"none": (None, None),
              "some": (np.array([0, 1, 5, 2, 9], np.int32), np.array([0, 1, 0, 2, 3, 1, 4], np.int32)),
              "all of query 0": (np.array([7, 1, 2, 3, 4], np.int32), np.full(7, 7, np.int32))}
    return (qt, ql, ct, cl), groups, {k: M.host_lcs(qt, ql, ct, cl, *v) for k, v in groups.items()}


def test_the_lcs_case_holds_what_it_is_meant_to(lcs_case):
    _, _, host = lcs_case
    L, ie, je = M.unpack(host["none"][0])
    assert L[1, 3] == 64 and (ie[1, 3], je[1, 3]) == (63, 63)           # all equal: min(Mq, Mc), at the first cell
    assert L[2, 5] == 12 and (ie[2, 5], je[2, 5]) == (119, 128)         # the run at the very end of both rows
    assert host["none"][1][2, 9] == 10                                  # and the one at the very start
    assert L[3, 4] == 30 and (ie[3, 4], je[3, 4]) == (29, 64)           # x alone: not x + y across the wrap
    assert (L[:, 0] == 0).all() and L[4, 1] == 1 and L[0].max() > 8
    Ls = M.unpack(host["some"][0])[0]
    assert Ls[0, 0] == Ls[0, 2] == Ls[1, 1] == Ls[1, 5] == Ls[3, 3] == 0 and (Ls[2] == L[2]).all() and Ls[1, 3] == 64
    assert not host["all of query 0"][0][0].any() and not host["all of query 0"][1][0].any()
    assert host["all of query 0"][0][1:].any()


@pytest.mark.parametrize("which", ["none", "some", "all of query 0"])
def test_motif_lcs_equals_the_host(lcs_case, which):
    rows, groups, host = lcs_case
    packed, reach = device_lcs(*rows, *groups[which])
    assert (packed == host[which][0]).all()
    assert (reach == host[which][1]).all()


def test_motif_lcs_replayed_from_a_graph_leaves_the_same_bits(lcs_case):
    rows, groups, host = lcs_case
    packed, reach = device_lcs(*rows, *groups["some"], graph=True)
    assert (packed == host["some"][0]).all() and (reach == host["some"][1]).all()


def test_motif_lcs_over_more_than_one_corpus_tile():
    tile = ops.motif_corpus_tile()
    g = np.random.default_rng(37)
    T, Nc = 40, tile + 5
    qs = [g.integers(0, 3, g.integers(0, T)) for _ in range(5)]
    cs = [g.integers(0, 3, g.integers(0, T)) for _ in range(Nc)]
    qt, ql = MC.token_rows(qs, T)
    ct, cl = MC.token_rows(cs, T)
    qg, cg = g.integers(0, 6, 5).astype(np.int32), g.integers(0, 6, Nc).astype(np.int32)
    want_p, want_r = M.host_lcs(qt, ql, ct, cl, qg, cg)
    packed, reach = device_lcs(qt, ql, ct, cl, qg, cg)
    assert (packed == want_p).all() and (reach == want_r).all()
    # lengths are what bounds a row: what lies behind them is never matched
    qt2, ct2 = qt.copy(), ct.copy()
    qt2[qt2 == M.PAD], ct2[ct2 == M.PAD] = 1, 1
    packed, reach = device_lcs(qt2, ql, ct2, cl, qg, cg)
    assert (packed == want_p).all() and (reach == want_r).all()


def test_motif_lcs_at_the_longest_row():
    """T = 4096: the kernel's largest LDS footprint and the largest positions the packed value holds."""
    g = np.random.default_rng(4096)
    T = ops.MOTIF_MAX_T
    a = g.integers(0, 3, T - 1)
    qt, ql = MC.token_rows([a], T)
    ct, cl = MC.token_rows([a, g.integers(0, 3, 70)], T)
    want_p, want_r = M.host_lcs(qt, ql, ct, cl)
    assert M.unpack(want_p)[0][0, 0] == T - 1 and M.unpack(want_p)[1][0, 0] == T - 2
    packed, reach = device_lcs(qt, ql, ct, cl)
    assert (packed == want_p).all() and (reach == want_r).all()


def test_motif_rank_equals_the_host_with_ties_and_a_short_corpus():
    g = np.random.default_rng(9)
    for Nc, k in ((300, 5), (4, 7), (1, 1), (700, 64)):
        p = g.integers(0, 6, (3, Nc)).astype(np.int64) << 32
        p[1] = 0
        want_v, want_i = M.host_rank(p, k)
        vals = torch.full((3, k), -5, dtype=torch.int64, device="cuda")
        idx = torch.full((3, k), -5, dtype=torch.int32, device="cuda")
        ops.motif_rank(dev(p), k, vals, idx)
        torch.cuda.synchronize()
        assert (vals.cpu().numpy() == want_v).all() and (idx.cpu().numpy() == want_i).all(), (Nc, k)


@pytest.fixture(scope="module")
def pieces():
    g = np.random.default_rng(21)
    T = 96
    corpus = [MC.walk_events(g, T, rests=0.1) for _ in range(9)]
    query = [MC.walk_events(g, int(n), rests=0.1) for n in (96, 96, 40, 1, 96, 70, 96)]
    query[0][50:66] = corpus[1][20:36]
    query[0][50:66, 0] += np.where(query[0][50:66, 1] >= 0, 3, 0)
    query[4][:30] = corpus[8][60:90]
    return MC.rolls_of(query, T), MC.rolls_of(corpus, T)


@pytest.mark.parametrize("groups", [False, True])
def test_match_gives_the_same_result_in_batches_of_2_and_64_and_on_the_host(pieces, groups):
    q, c = pieces
    qg = cg = None
    if groups:
        qg, cg = np.array([0, 1, 2, 3, 8, 5, 6], np.int32), np.arange(9, dtype=np.int32)
    want = M.host_match(q, c, qg, cg, top=3)
    assert M.unpack(want.vals)[0][0, 0] >= 10 and (M.unpack(want.vals)[0][4, 0] >= 20) != groups
    for batch in (2, 64):
        got = M.Motifs(0, 3, batch).match(q, c, qg, cg)
        for name in ("q_tokens", "q_len", "c_tokens", "c_len", "vals", "idx", "reach"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (batch, name)


def test_the_tool_on_the_device_writes_what_cpu_writes(tmp_path, capsys):
    files = MC.write_midi_cases(str(tmp_path / "midi"))
    reports = {}
    for flag in ("--cpu", None):
        out = str(tmp_path / f"motifs{flag}.json")
        argv = [files["b"], files["c"], "--corpus", files["a"], files["c"], "--baseline", files["a"], "--max-notes", "24", "--hop", "8",
                "--batch", "3", "--out", out] + ([flag] if flag else [])
        assert M.main(argv) == 0, capsys.readouterr().err
        reports[flag] = json.load(open(out))
    assert reports["--cpu"].pop("device") is False and reports[None].pop("device") is True
    assert reports[None] == reports["--cpu"]
    assert len(reports[None]["rows"]) > 3 and reports[None]["summary"]["max_longest"] >= 15
    # and --self
    for flag in ("--cpu", None):
        out = str(tmp_path / f"self{flag}.json")
        assert M.main(["--corpus", str(tmp_path / "midi"), "--self", "--out", out] + ([flag] if flag else [])) == 0
        reports[flag] = json.load(open(out))
    reports["--cpu"].pop("device"), reports[None].pop("device")
    assert reports[None] == reports["--cpu"] and len(reports[None]["pairs"]) == 1


def test_bad_arguments_are_rejected_before_any_launch():
    """As tests/test_abi.py does it: non-null dummy addresses, nothing launches."""
    from melo_gan_amd import _lib
    lib = _lib.load()
    x, t, n, p, r = 256, 512, 1024, 2048, 4096

    def refused(rc, word):
        assert rc == -1 and word in lib.mg_last_error(), (rc, lib.mg_last_error())

    refused(lib.mg_motif_tokens(None, 1, 8, 0, t, n, None), b"null")
    refused(lib.mg_motif_tokens(x, 1, 8, 0, None, n, None), b"null")
    refused(lib.mg_motif_tokens(x, 1, 8, 0, t, None, None), b"null")
    refused(lib.mg_motif_tokens(x, 0, 8, 0, t, n, None), b"N = 0")
    for T in (0, -1, ops.MOTIF_MAX_T + 1):
        refused(lib.mg_motif_tokens(x, 1, T, 0, t, n, None), b"T = ")
        refused(lib.mg_motif_lcs(t, n, 1, t, n, 1, T, None, None, p, r, None), b"T = ")
    for mode in (-1, 2):
        refused(lib.mg_motif_tokens(x, 1, 8, mode, t, n, None), b"mode")
    refused(lib.mg_motif_tokens(x, 1, 8, 0, t + 1, n, None), b"aligned")
    refused(lib.mg_motif_tokens(x + 8, 1, 8, 0, t, n, None), b"aligned")
    lcs = lambda **k: lib.mg_motif_lcs(*[k.get(a, d) for a, d in (("qt", t), ("ql", n), ("Nq", 1), ("ct", t), ("cl", n), ("Nc", 1),  # noqa: E731
                                                                   ("T", 8), ("qg", None), ("cg", None), ("packed", p), ("reach", r))], None)
    for name in ("qt", "ql", "ct", "cl", "packed", "reach"):
        refused(lcs(**{name: None}), b"null")
    refused(lcs(qt=t + 1), b"2-byte")
    refused(lcs(ct=t + 1), b"2-byte")
    refused(lcs(ql=n + 2), b"aligned")
    refused(lcs(packed=p + 4), b"aligned")
    refused(lcs(qg=n), b"go together")
    refused(lcs(Nq=0), b"Nq")
    refused(lcs(Nq=65536), b"Nq")
    refused(lcs(Nc=0), b"Nc")
    refused(lib.mg_motif_rank(None, 1, 1, 1, p, n, None), b"null")
    refused(lib.mg_motif_rank(p, 1, 1, 1, None, n, None), b"null")
    refused(lib.mg_motif_rank(p, 1, 1, 0, p, n, None), b"k = 0")
    refused(lib.mg_motif_rank(p, 1, 1, ops.MOTIF_MAX_K + 1, p, n, None), b"k = ")
    refused(lib.mg_motif_rank(p, 1, 0, 1, p, n, None), b"Nc")
    refused(lib.mg_motif_rank(p + 4, 1, 1, 1, p, n, None), b"aligned")
    # and the wrappers check shapes and dtypes on the host
    tok = torch.zeros(2, 8, dtype=torch.uint16, device="cuda")
    ln = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.motif_tokens(torch.zeros(2, 8, 4, device="cuda"), 2)
    with pytest.raises(ValueError):
        ops.motif_tokens(torch.zeros(2, ops.MOTIF_MAX_T + 1, 4, device="cuda"), 0)
    with pytest.raises(ValueError):
        ops.motif_lcs(tok, ln, torch.zeros(2, 9, dtype=torch.uint16, device="cuda"), ln)
    with pytest.raises(ValueError):
        ops.motif_lcs(tok, ln, tok, ln, q_groups=ln)
    with pytest.raises(ValueError):
        ops.motif_lcs(tok.to(torch.int32), ln, tok, ln)
    with pytest.raises(ValueError):
        ops.motif_rank(torch.zeros(2, 3, dtype=torch.int64, device="cuda"), 0)
