"""csrc/conv_thin.hip -- thin_in_kernel and thin_out_kernel<TR2, NMAX>, the first and last layer of every network at
NOTE_DIM = 4 -- pinned to fp64, element by element: |got - ref| <= (n + 4 + k_epi) 2^-24 M + eps_abs with n = K Cin, the
references of tests/window_ref.py / tests/stride2_ref.py (W.thin names the one behind each entry point) and no slack for
thin_out's 16-lane shuffle tree or its two channel passes (any tree over n products has at most n - 1 additions on a path).

The shape tables are plain data in tests/thin_bf16_tables.py; tests/test_thin_bf16_ref.py shows on the host which path each
row reaches (route, NMAX, rpt = 1 / 2 / 4 / 8, the second channel pass, the 16-byte and the scalar loads and stores).  Every
case asserts the route (mg_conv_thin_route on the tensors used, and the symbol the launch hook reports) before it trusts a
number, reads x out of a canvas of non-zero values or from a view that starts off the 16-byte grid, writes into NaN-prefilled
outputs inside sentinel rows, and checks every element; rows of a padded y beyond Tout must keep their prefill bit for bit.
The fp64 references are evaluated on the device.

Each test prints the worst error / bound ratio of its section (pytest -s shows it).  Measured on an MI355X: see DESIGN.md
section 2."""
import pytest
import torch

import stride2_ref as S
import thin_bf16_tables as T
import window_ref as W
import test_window_contract_gpu as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


@pytest.fixture
def hook(ops):
    rec = WC._Symbols()
    ops.set_launch_hook(rec)
    try:
        yield rec
    finally:
        ops.set_launch_hook(None)


class Worst(WC.Worst):
    def report(self, capsys):
        with capsys.disabled():
            print(f"\n[thin contract] {self.section}: {self.n} checks, worst error / bound = {self.r:.4f} ({self.what})")


class GuardedOff4(S.Guarded):
    """S.Guarded whose output starts 4 bytes past a 16-byte boundary."""

    def __init__(self, shape, fill=float("nan"), rows=64):
        n = 1
        for s in shape:
            n *= s
        self.pad = rows * shape[-1]
        self.canvas = torch.full((n + 2 * self.pad + 1,), self.SENTINEL, device="cuda")[1:]
        self.t = self.canvas[self.pad:self.pad + n].view(*shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 4


SYMS = {1: "thin_in_kernel", 2: "thin_out_kernel<%s,4>", 3: "thin_out_kernel<%s,8>"}


def symbol(route, transposed):
    s = SYMS[route]
    return s % ("true" if transposed else "false") if "%s" in s else s


def launch(ops, case, x, w, y, **epi):
    e, stride = case[0], case[6]
    if e == "fwd":
        return ops.conv1d_fwd(x, w, y, stride, **epi)
    if e == "convT_dgrad":
        return ops.convT1d_dgrad(x, w, y, **epi)
    if e == "dgrad1":
        return ops.conv1d_dgrad(x, w, y, 1, **epi)
    if e == "convT_fwd":
        return ops.convT1d_fwd(x, w, y, **epi)
    return ops.conv1d_dgrad(x, w, y, 2, **epi)


def problem(case, seed):
    """x (read from a canvas of non-zero values, or misaligned), w and the fp64 (value, M) of one table row."""
    e, B, Tin, C, N, K, stride, flags = case
    x = WC.rnd(B, Tin, C, seed=seed)
    x = WC.off4(x) if "xoff" in flags else WC._in_canvas(x)[0]
    w = WC.rnd(*T.ENTRIES[e][2](C, N, K), seed=seed + 1, scale=0.3)
    Tout = T.tout(e, Tin, K, stride, flags)
    return x, w, Tout, W.thin(e, x, w, K, stride, Tout)


def expect_route(case, x):
    """The route the tables claim, checked against mg_conv_thin_route on the tensor the launch gets."""
    from melo_gan_amd import _lib
    e, B, Tin, C, N, K, stride, flags = case
    tr = T.ENTRIES[e][0]
    want = T.route(C, N, K, stride, tr, x.data_ptr() % 16 == 0)
    got = _lib.load().mg_conv_thin_route(x.data_ptr(), Tin * C, C, N, K, stride, 1 if tr else 0)
    assert got == want, (T.case_id(case), got, want)
    return want, tr


def run_case(ops, hook, worst, case, seed, want_route):
    e, B, Tin, C, N, K, stride, flags = case
    what = T.case_id(case)
    x, w, Tout, acc = problem(case, seed)
    route, tr = expect_route(case, x)
    assert route in want_route, (what, route)
    bias = WC.rnd(N, seed=seed + 2)
    Ty = Tout + 3 if "ypad" in flags else Tout
    fill = 7.0 if "ypad" in flags else float("nan")
    y = GuardedOff4((B, Ty, N), fill=fill) if "yoff" in flags else S.Guarded((B, Ty, N), fill=fill)
    if route == 1:
        assert T.vec_out(N, Ty, "yoff" not in flags) == (N % 4 == 0 and "yoff" not in flags)
    hook.seen.clear()
    launch(ops, case, x, w, y.t, bias=bias)
    if route:
        assert hook.seen == [symbol(route, tr)], (what, hook.seen)
    else:
        assert len(hook.seen) == 1 and hook.seen[0].startswith("conv_wgemm_kernel<"), (what, hook.seen)
    worst.check(y.t[:, :Tout], W.Ref(acc[0], acc[1], K * C).epilogue(bias=bias), what)
    y.check(what)
    if "ypad" in flags:
        assert bool((y.t[:, Tout:] == 7.0).all()), what + ": rows beyond Tout written"
    return route


def test_thin_in_edge_shapes(ops, hook, capsys):
    worst = Worst("a. thin_in_kernel, edge shapes")
    for i, case in enumerate(T.THIN_IN):
        run_case(ops, hook, worst, case, 10 * i, (1,))
    worst.report(capsys)


def test_thin_out_edge_shapes(ops, hook, capsys):
    worst, seen = Worst("b. thin_out_kernel, edge shapes"), set()
    for i, case in enumerate(T.THIN_OUT):
        r = run_case(ops, hook, worst, case, 10 * i + 3, (0,) if case[3] > T.THIN_OUT_CMAX else (2, 3))
        seen.add((T.ENTRIES[case[0]][0], r))
    assert seen >= {(tr, r) for tr in (True, False) for r in (0, 2, 3)}, seen
    worst.report(capsys)


@pytest.mark.parametrize("case", T.RPT, ids=[T.case_id(c) for c in T.RPT])
def test_thin_out_positions_loop(ops, hook, capsys, case):
    """rpt = 2 / 4 / 8: the last workgroup holds a partly live block and wholly dead iterations."""
    rows = case[1] * case[2]
    assert T.rpt(rows) == {32789: 2, 65573: 4, 131125: 8, 32805: 2}[rows]
    worst = Worst(f"c. thin_out_kernel rpt={T.rpt(rows)} {case[0]}")
    run_case(ops, hook, worst, case, rows % 97, (2,))
    worst.report(capsys)


@pytest.mark.parametrize("case", T.EPILOGUE, ids=[T.case_id(c) for c in T.EPILOGUE])
def test_every_epilogue_piece(ops, hook, capsys, case):
    e, B, Tin, C, N, K, stride, flags = case
    x, w, Tout, acc = problem(case, 5)
    route, tr = expect_route(case, x)
    assert route in (1, 2, 3)
    worst = Worst(f"d. epilogues in {symbol(route, tr)} ({e})")
    shape = (B, Tout, N)
    for misalign in (False, True):
        for name, epi, repi in WC._epilogue_cases(ops, shape, N, misalign=misalign):
            if misalign and name in ("bias", "scale/shift", "accumulate"):
                continue                                  # nothing elementwise to misalign
            hook.seen.clear()
            WC._run_epilogue_case(lambda y, **kw: launch(ops, case, x, w, y, **kw), shape, epi, repi, acc, K * C, worst,
                                  f"{name} misalign={misalign} {T.case_id(case)}", misalign)
            assert hook.seen == [symbol(route, tr)], hook.seen
    worst.report(capsys)


def test_stride2_three_taps_on_a_wide_input_is_refused_on_the_host(ops, hook):
    """thin_in takes K = 3 at stride 2 (Cin <= 8: rows of THIN_IN); with a wide input nothing does -- the library says so
    before any launch and writes nothing."""
    x, w = WC.rnd(2, 20, 16, seed=1), WC.rnd(4, 16, 3, seed=2)
    y = S.Guarded((2, 10, 4))
    with pytest.raises(RuntimeError, match="K=5"):
        ops.conv1d_fwd(x, w, y.t, 2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all())
    y.check("refused")
    with pytest.raises(RuntimeError, match="flip"):         # a flipped gather is stride 1 only
        ops.conv_gather(WC.rnd(2, 20, 4, seed=1), WC.rnd(4, 8, 5, seed=2), y.t, 4, 5, 2, 5, 20, flip=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all())
