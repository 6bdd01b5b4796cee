"""CPU-only: the C-ABI library is built, loads, and exports every symbol include/melo_gan_hip.h
declares (no compute calls without a GPU); the ctypes signature table covers the header."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_functions():
    src = open(os.path.join(ROOT, "include", "melo_gan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert lib.mg_version() >= 100
    assert set(_lib.SIGNATURES) <= set(names), set(_lib.SIGNATURES) - set(names)


def test_bad_arguments_are_rejected_before_any_launch():
    """Argument validation happens before any launch, so it can be exercised without a GPU."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    lib = _lib.load()
    rc = lib.mg_conv1d_gather(None, None, None, 1, 1, 1, 1, 5, 1, 0, 5, 1, 0, 0, None, None, 0, 0, None)
    assert rc == -1 and b"null" in lib.mg_last_error()
    rc = lib.mg_wgrad(None, None, 0, None, None, 0, None, None, 0, 1, 1, 1, 1, 1, 1, None, 0, None)
    assert rc == -1
    assert lib.mg_wgrad_workspace_bytes(64, 64, 5, 8, 32) > 0
    # the multi-job entry points: job count limits, null tensors, malformed rows
    assert lib.mg_wgrad_multi(None, 1, 1, 1, None, 0, None) == -1
    jobs = (_lib.WgradJob * 1)()
    assert lib.mg_wgrad_multi(jobs, 0, 1, 1, None, 0, None) == -1
    assert lib.mg_wgrad_multi(jobs, _lib.MAX_WGRAD_JOBS + 1, 1, 1, None, 0, None) == -1
    assert lib.mg_wgrad_multi(jobs, 1, 1, 1, None, 0, None) == -1 and b"segment 0" in lib.mg_last_error()
    st = (_lib.StageJob * 1)()
    assert lib.mg_stage_rows(st, 0, 4, None) == -1 and lib.mg_stage_rows(st, _lib.MAX_STAGE_JOBS + 1, 4, None) == -1
    assert lib.mg_stage_rows(st, 1, 4, None) == -1                      # null source / destination
    st[0].src, st[0].dst, st[0].row_bytes, st[0].src_rows = 256, 512, 6, 8
    assert lib.mg_stage_rows(st, 1, 4, None) == -1                      # rows must be multiples of 4 bytes
    st[0].row_bytes, st[0].dst_pitch = 8, 4
    assert lib.mg_stage_rows(st, 1, 4, None) == -1 and b"dst_pitch" in lib.mg_last_error()
    st[0].dst_pitch, st[0].src_rows = 0, 2
    assert lib.mg_stage_rows(st, 1, 4, None) == -1                      # unindexed source shorter than the batch
    assert lib.mg_dhead_fwd_bwd(None, None, None, None, None, None, None, None, 4, 4, 8, 8, 0, None) == -1
    # empty shapes (non-null dummy addresses): R = 0 used to reach the launch plan of mg_bn_train_bwd, which divides by the rows per slice
    q = 256
    for R_, C_ in ((0, 64), (64, 0)):
        assert lib.mg_bn_train_bwd(q, q, q, q, R_, C_, q, None, q, q, q, q, 1, q, 1 << 24, None) == -1 and b"mg_bn_train_bwd" in lib.mg_last_error()
        assert lib.mg_bn_eval_fwd(q, q, R_, C_, q, q, q, q, 1e-5, 0, None) == -1 and b"mg_bn_eval_fwd" in lib.mg_last_error()
    for B_, D_ in ((0, 6), (4, 0), (4, 65)):
        assert lib.mg_layernorm_bwd_params(q, q, q, q, B_, D_, None) == -1 and b"mg_layernorm_bwd_params" in lib.mg_last_error()


def test_lds_pad_outside_its_range_is_rejected_on_the_host():
    """The occupancy cap is a launch argument of the two window-GEMM entry points that take it: 0..120 KiB, checked before
    any launch (non-null dummy addresses, so that the null-tensor check does not answer first)."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    lib = _lib.load()
    x, w, y = 256, 512, 1024
    for pad in (-1, 120 * 1024 + 1):
        rc = lib.mg_conv1d_gather(x, w, y, 4, 256, 64, 128, 3, 1, 0, 192, 3, 0, 0, None, None, 0, pad, None)
        assert rc == -1 and b"lds_pad" in lib.mg_last_error(), pad
        assert lib.mg_conv1d_wino3(x, w, y, 4, 256, 64, 128, None, pad, None) == -1 and b"lds_pad" in lib.mg_last_error(), pad


def test_riders_are_checked_by_their_family_entry_point():
    """Every kernel family has ONE entry point whose riders are nullable arguments; the rules between riders are checked
    there, before any launch (non-null dummy addresses; nothing here launches)."""
    import ctypes as C
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    lib = _lib.load()
    x, w, y, q, r = 256, 512, 1024, 2048, 4096
    # mg_conv16: no extra and null tensors; the temporal mean of an accumulating launch
    assert lib.mg_conv16(None, None, None, 4, 64, 64, 128, 0, 0, 0, 0, None, None, None) == -1 and b"null" in lib.mg_last_error()
    epi, ex = _lib.Epilogue(), _lib.Conv16Extra()
    epi.accumulate, ex.pool, ex.pool_scale = 1, q, 1.0
    assert lib.mg_conv16_poolable(4, 64, 64, 128)
    rc = lib.mg_conv16(x, w, y, 4, 64, 64, 128, 0, 0, 0, 0, C.byref(epi), C.byref(ex), None)
    assert rc == -1 and b"mean of an accumulating" in lib.mg_last_error()
    # mg_rng_fill: a second Adam state without / equal to the first; staging jobs without both states
    draw = (x, 16, None, 0, None, 0, None, 0, 0.0, 1, w)
    tail = (None, 0, 0, None, 0, None, None)
    assert lib.mg_rng_fill(*draw, None, q, 0.9, 0.99, *tail) == -1 and b"adam_state" in lib.mg_last_error()
    assert lib.mg_rng_fill(*draw, q, q, 0.9, 0.99, *tail) == -1 and b"adam_state" in lib.mg_last_error()
    st = (_lib.StageJob * 1)()
    st[0].src, st[0].dst, st[0].row_bytes, st[0].src_rows = 256, 512, 16, 16
    for states in ((None, None), (q, None)):
        assert lib.mg_rng_fill(*draw, *states, 0.9, 0.99, st, 1, 8, None, 16, r, None) == -1, states
        assert b"both adam states" in lib.mg_last_error(), states
    # mg_adam_flat: a WQ table that is missing or too long
    adam = (x, w, y, q, 64, 1e-3, 0.9, 0.99, 1e-8, 0.0, r, 1.0, None, 0, None)
    assert lib.mg_adam_flat(*adam, None, 1, None) == -1 and b"table" in lib.mg_last_error()
    tab = (_lib.WqEntry * (_lib.MAX_WQ_ENTRIES + 1))()
    assert lib.mg_adam_flat(*adam, tab, _lib.MAX_WQ_ENTRIES + 1, None) == -1 and b"table" in lib.mg_last_error()
    # mg_graph_end: 1..8 executables
    out = (C.c_void_p * 9)()
    for n in (0, 9):
        assert lib.mg_graph_end(None, out, n) == -1 and b"1..8" in lib.mg_last_error(), n


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    with pytest.raises(ValueError):
        ops.conv1d_fwd(torch.zeros(1, 8, 4), torch.zeros(8, 4, 5), torch.zeros(1, 4, 8), 2)


def test_loading_the_library_before_torch_leaves_one_hip_runtime():
    """build() loads the library before anything has imported torch.  torch's wheel carries its own libamdhip64.so; if the
    library pulled in the system's copy first, the process would hold two HIP runtimes and the second to open the device
    would find none (smoke() after build() in one process).  _lib.load() therefore imports torch first: checked in a fresh
    process by counting the runtimes mapped."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import melo_gan_amd\n"
            "from melo_gan_amd import _lib\n"
            "_lib.load()\n"
            "import torch\n"
            "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout
