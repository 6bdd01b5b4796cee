"""Shape tables of tests/test_thin_contract_gpu.py and tests/test_bf16_contract_gpu.py, as plain data, with the host
side rules of csrc/conv_thin.hip and csrc/conv_bf16.hip restated in Python (route, rpt, x4, vec_out, nchunks) so that
tests/test_thin_bf16_ref.py can show without a GPU which path every row reaches.  A plain helper module; nothing here is
collected.

A thin case is (entry, B, T, C, N, K, stride, flags): x is (B, T, C), the output has N channels, `entry` names the ops.py
entry point (below), flags is a set out of "xoff" (x starts 4 bytes past a 16-byte boundary), "yoff" (y does), "ypad" (y
has three more rows than Tout), "odd" (stride-2 data gradient onto an odd length, Tout = 2 T - 1)."""

TK, TC, THIN_OUT_CMAX = 5, 8, 256          # conv_thin.hip: taps, thin channels, widest input of thin_out

# entry -> (transposed, flip, weight shape as a function of (C, N, K)); x always (B, T, C), the result (B, Tout, N)
ENTRIES = {
    "fwd":         (False, False, lambda C, N, K: (N, C, K)),      # ops.conv1d_fwd(x, w (N, C, K), y, stride)
    "convT_dgrad": (False, False, lambda C, N, K: (N, C, K)),      # ops.convT1d_dgrad(dy, w (N, C, 5), dx): a stride-2 gather
    "dgrad1":      (False, True, lambda C, N, K: (C, N, K)),       # ops.conv1d_dgrad(dy, w (C, N, K), dx, 1)
    "convT_fwd":   (True, False, lambda C, N, K: (C, N, K)),       # ops.convT1d_fwd(x, w (C, N, 5), y)
    "dgrad2":      (True, False, lambda C, N, K: (C, N, K)),       # ops.conv1d_dgrad(dy, w (C, N, 5), dx, 2)
}


def tout(entry, T, K, stride, flags=()):
    if ENTRIES[entry][0]:
        return 2 * T - (1 if "odd" in flags else 0)
    return (T + 2 * ((K - 1) // 2) - K) // stride + 1


def route(C, N, K, stride, transposed, x_aligned=True):
    """mg_conv_thin_route: 0 none, 1 thin_in, 2 / 3 thin_out with 4 / 8 column slots (x of one (B, T, C) tensor: xbs = T C)."""
    if K > TK or K < 3:
        return 0
    if not transposed and C <= TC:
        return 1
    vec = C % 4 == 0 and x_aligned
    if N <= TC and vec and C <= THIN_OUT_CMAX and (K == 5 if transposed else stride == 1):
        return 2 if N <= 4 else 3
    return 0


def rpt(rows):
    """launch_thin_out: positions per slot of a workgroup."""
    blocks, r = -(-rows // 16), 1
    while r < 8 and blocks // (r * 2) >= 1024:
        r *= 2
    return r


def x4(C, T, x_aligned=True):
    """thin_in_kernel's 16-byte window loads (else: scalar loads)."""
    return C == 4 and (T * C) % 4 == 0 and x_aligned


def vec_out(N, Ty, y_aligned=True):
    """thin_in_kernel's 16-byte stores."""
    return N % 4 == 0 and (Ty * N) % 4 == 0 and y_aligned


def nchunks(Cin):
    return Cin // 32


def case_id(c):
    e, B, T, C, N, K, s, fl = c
    return f"{e}-B{B}-T{T}-C{C}-N{N}-K{K}-s{s}" + "".join("-" + f for f in sorted(fl))


X, Y, P, O = "xoff", "yoff", "ypad", "odd"
# ---- thin_in: C <= 8 ------------------------------------------------------------------------------------------------
THIN_IN = [
    ("fwd", 1, 1, 1, 4, 3, 1, set()),             # one output row
    ("fwd", 3, 5, 3, 6, 5, 1, set()),             # 15 rows; N % 4 != 0: a partial column quad, scalar stores
    ("fwd", 1, 16, 4, 64, 3, 1, set()),           # 16 rows: exactly one block; the 16-byte loads
    ("fwd", 1, 17, 8, 68, 5, 1, set()),           # 17 rows; a second blockIdx.y holding one quad
    ("fwd", 7, 5, 4, 100, 5, 1, set()),           # Tout = 5, B = 7: blocks cross sample boundaries; second blockIdx.y, 9 quads
    ("fwd", 2, 9, 4, 70, 5, 1, set()),            # a partial column quad (columns 68, 69 of 68..71) on the second blockIdx.y
    ("fwd", 2, 9, 4, 64, 5, 1, {X}),              # Cin = 4 off the 16-byte grid: the scalar loads
    ("fwd", 2, 9, 4, 64, 3, 1, {Y}),              # vec_out off
    ("fwd", 3, 6, 4, 68, 5, 1, {P}),
    ("fwd", 2, 9, 1, 100, 3, 1, {P, X}),
    ("fwd", 2, 1, 4, 64, 5, 2, set()),            # stride 2: T = 1, 2, even, odd
    ("fwd", 2, 2, 3, 6, 5, 2, set()),
    ("fwd", 3, 20, 4, 100, 5, 2, set()),
    ("fwd", 5, 21, 8, 68, 5, 2, {P}),
    ("fwd", 2, 21, 4, 64, 5, 2, {X, Y}),
    ("fwd", 3, 20, 4, 68, 3, 2, set()),           # K = 3 at stride 2 (no layer; the route admits it)
    ("fwd", 2, 21, 3, 6, 3, 2, set()),
    ("convT_dgrad", 3, 32, 4, 64, 5, 2, set()),
    ("convT_dgrad", 2, 18, 3, 100, 5, 2, set()),
    ("convT_dgrad", 7, 10, 8, 4, 5, 2, {Y}),      # Tout = 5, B = 7
    ("dgrad1", 2, 17, 4, 64, 3, 1, set()),        # flip = 1
    ("dgrad1", 7, 5, 8, 68, 5, 1, set()),
    ("dgrad1", 1, 33, 3, 6, 5, 1, set()),
    ("dgrad1", 2, 9, 4, 100, 3, 1, {X}),
    ("dgrad1", 1, 15, 1, 4, 3, 1, {P}),
]

# ---- thin_out: N <= 8, C wide ---------------------------------------------------------------------------------------
THIN_OUT = [
    ("convT_fwd", 1, 1, 4, 1, 5, 2, set()),       # one position; one live lane; NMAX = 4
    ("convT_fwd", 3, 5, 16, 3, 5, 2, set()),      # 15 positions
    ("convT_fwd", 1, 16, 64, 4, 5, 2, set()),     # 16 positions; all lanes, one pass
    ("convT_fwd", 1, 17, 68, 5, 5, 2, set()),     # 17; second channel pass with lane 0 only; NMAX = 8
    ("convT_fwd", 7, 5, 128, 8, 5, 2, set()),     # a sample boundary inside a block
    ("convT_fwd", 2, 8, 256, 4, 5, 2, {P}),       # the widest input; padded Ty
    ("convT_fwd", 2, 8, 260, 4, 5, 2, set()),     # routes to 0 (the MFMA tile kernel)
    ("dgrad2", 3, 9, 68, 4, 5, 2, {O}),           # Tout = 2 Tin - 1
    ("dgrad2", 2, 1, 16, 8, 5, 2, {O}),           # Tin = 1 -> one output row
    ("dgrad2", 7, 5, 64, 3, 5, 2, {P}),           # (conv1d_dgrad reads "odd" off dx's length: padded means even)
    ("dgrad2", 2, 10, 128, 5, 5, 2, {O}),
    ("dgrad1", 1, 1, 16, 4, 3, 1, set()),         # gather form, flipped
    ("dgrad1", 3, 5, 68, 8, 5, 1, set()),
    ("dgrad1", 7, 5, 64, 1, 3, 1, set()),
    ("dgrad1", 1, 17, 256, 5, 5, 1, {P}),
    ("dgrad1", 2, 9, 260, 4, 3, 1, set()),        # routes to 0
    ("fwd", 1, 16, 16, 3, 5, 1, set()),           # gather form, not flipped
    ("fwd", 1, 17, 68, 4, 3, 1, set()),
    ("fwd", 7, 5, 128, 8, 5, 1, set()),
    ("fwd", 3, 5, 4 * 3, 5, 3, 1, {P}),           # Cin = 12: three live lanes
]

# ---- the rpt loop: positions 2^15 + 21, 2^16 + 37, 2^17 + 53 (the last workgroup: a partly live block, then dead iterations)
RPT = [
    ("convT_fwd", 1, 32789, 8, 4, 5, 2, set()), ("fwd", 1, 32789, 16, 4, 5, 1, set()),
    ("dgrad2", 23, 2851, 16, 4, 5, 2, set()), ("dgrad1", 23, 2851, 12, 4, 3, 1, set()),
    ("convT_fwd", 125, 1049, 12, 4, 5, 2, set()), ("fwd", 125, 1049, 16, 4, 3, 1, set()),
    ("dgrad2", 45, 729, 8, 4, 5, 2, {O}),         # 2^15 + 37 positions: 2051 blocks at rpt = 2, so a dead iteration there too
]

# ---- every epilogue piece: thin_in (vector and scalar stores, two column blocks), thin_out transposed and gathered
EPILOGUE = [("fwd", 3, 11, 4, 68, 5, 1, set()), ("dgrad1", 2, 9, 3, 6, 3, 1, set()), ("convT_fwd", 3, 7, 68, 4, 5, 2, set()),
            ("fwd", 3, 11, 68, 5, 3, 1, set())]

# ---- conv_bf16_kernel: (B, T, Cin, N) ---------------------------------------------------------------------------------
BF16_SHAPES = [
    (1, 128, 32, 64),         # one tile, one chunk
    (2, 128, 64, 64),         # tile edge = sample edge: the halo is zero, not the neighbour's rows
    (1, 256, 96, 128),        # halo from inside the sequence, three chunks (the break in the two-chunk ring), second column tile
    (3, 128, 160, 64),        # five chunks
    (2, 256, 256, 192),       # eight chunks
]
BF16_INSTANCES = [(K, xf32, yf32) for K in (3, 5) for xf32 in (False, True) for yf32 in (False, True)]
BF16_EPI_SHAPES = [(2, 128, 64, 64), (1, 256, 96, 128)]
MEANT_FWD = [(B, T, C) for T, B in ((1, 3), (5, 2), (13, 2), (17, 3), (29, 2), (256, 2)) for C in (8, 64, 72)]
MEANT_BWD = [(3, 37, 8), (2, 29, 72), (5, 123, 72)]          # B T C / 8 not a multiple of 256 threads (2048 elements)
# wb_relayout: (N, Cc, K, layout) with layout "nck": (w_sn, w_sc) = (Cc K, K) on a (N, Cc, K) weight; "cnk": (K, N K) on a
# (Cc, N, K) weight (conv1d_dgrad: the image of the data gradient, with flip)
RELAYOUT = [(64, 32, 3, "nck"), (64, 96, 5, "nck"), (32, 64, 3, "cnk"), (96, 64, 5, "cnk"), (5, 7, 3, "nck"), (7, 5, 5, "cnk")]


def bf16_sym(K, xf32, yf32):
    b = lambda v: "true" if v else "false"  # noqa: E731
    return f"conv_bf16_kernel<{K},{b(xf32)},{b(yf32)}>"
