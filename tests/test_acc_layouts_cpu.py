"""CPU: the four accumulator families of ops.py (eval_acc, note_acc, vae_eval_acc, cls_eval) come from one description: the
views by name have the documented shapes and dtypes, together they address every 4-byte half-word of the accumulator exactly
once, `words` is the library's mg_*_acc_words, and every family refuses a short, a non-int64 and a non-contiguous tensor.
Then eval_pass.Packed: disjoint typed views, and the views of a copy read back what was written through the first set.
The library's host functions load without a device."""
import math

import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd import _lib, ops
from melo_gan_amd.eval_pass import Packed

I64, F64, F32, I32 = torch.int64, torch.float64, torch.float32, torch.int32


def eval_family(K, C):
    want = {"n": ((K,), I64), "conf_fake": ((K, K), I64), "conf_real": ((K, K), I64), "d_sum": ((2,), F64), "cls": ((2, 2, K), F64),
            "nsum": ((2, K, C), F64), "nsq": ((2, K, C), F64), "nmin": ((2, K, C), F32), "nmax": ((2, K, C), F32)}
    return ops.eval_acc_layout(K, C), lambda a: ops.eval_acc_views(a, K, C), want, _lib.load().mg_eval_acc_words(K, C), None


def note_family(K):
    shapes = {"counters": (8,), "pitch": (128,), "velocity": (128,), "dur16": (16,), "step16": (16,), "interval": (64,),
              "pctm": (12, 12)}
    assert dict(ops.NOTE_ACC_FIELDS) == shapes and [n for n, _ in ops.NOTE_ACC_FIELDS] == list(shapes)
    want = {k: ((2, K) + s, I64) for k, s in shapes.items()}
    return ops.note_acc_layout(K), lambda a: ops.note_acc_views(a, K), want, _lib.load().mg_note_acc_words(K), 504


def vae_family(K, Ld):
    want = {"c": ((K, 16), I64), "se": ((K, 4), F64), "ae": ((K, 4), F64), "beats_abs": ((K, 2), F64), "lat": ((K, 5, Ld), F64)}
    return (ops.vae_eval_acc_layout(K, Ld), lambda a: ops.vae_eval_acc_views(a, K, Ld), want,
            _lib.load().mg_vae_eval_acc_words(K, Ld), 26 + 5 * Ld)


def cls_family(K, nb, G):
    assert ops.CLS_INT_FIELDS == ("rows", "correct", "flipped", "confusion", "bin_count", "bin_correct")
    assert ops.CLS_FIELDS == ops.CLS_INT_FIELDS + ("ce", "brier", "conf", "margin", "bin_conf", "nll_T")
    tail = {"confusion": (K,), "bin_count": (nb,), "bin_correct": (nb,), "bin_conf": (nb,), "nll_T": (G,)}
    want = {k: ((K,) + tail.get(k, ()), I64 if k in ops.CLS_INT_FIELDS else F64) for k in ops.CLS_FIELDS}
    return (ops.cls_eval_layout(K, nb, G), lambda a: ops.cls_eval_views(a, K, nb, G), want,
            _lib.load().mg_cls_eval_acc_words(K, nb, G), 7 + K + 3 * nb + G)


FAMILIES = ([(eval_family, (K, C)) for K in (1, 4, 32) for C in (4, 8, 128)] + [(note_family, (K,)) for K in (1, 4, 32)] +
            [(vae_family, (K, Ld)) for K in (1, 4) for Ld in (1, 8, 1024)] +
            [(cls_family, (K, nb, G)) for K in (2, 16) for nb in (1, 15, 32) for G in (1, 64)])


@pytest.mark.parametrize("family,args", FAMILIES, ids=lambda v: v.__name__ if callable(v) else "-".join(map(str, v)))
def test_views_cover_the_accumulator_once(family, args):
    lay, views, want, lib_words, block = family(*args)
    words = lay["words"]
    assert words == lib_words and words > 0
    assert ("block" in lay) == (block is not None) and lay.get("block") == block
    assert set(lay) == set(want) | {"words"} | ({"block"} if block is not None else set())
    # every 4-byte half-word carries its own index
    acc = torch.arange(2 * words, dtype=I32).view(I64)
    v = views(acc)
    assert list(v) == list(want)                                          # by name, in the layout's order
    seen = []
    for name, (shape, dtype) in want.items():
        assert tuple(v[name].shape) == shape and v[name].dtype == dtype, (name, tuple(v[name].shape), v[name].dtype)
        assert v[name].data_ptr() >= acc.data_ptr() and v[name]._base is not None              # a view, not a copy
        halves = v[name].contiguous().view(-1).view(I32)
        assert halves.numel() * 4 == math.prod(shape) * v[name].element_size()
        seen.append(halves)
        # the layout's offset is where the first block's field starts
        assert (v[name].data_ptr() - acc.data_ptr()) == 8 * lay[name][0], name
    seen = torch.cat(seen)
    assert seen.numel() == 2 * words and torch.equal(torch.sort(seen).values, torch.arange(2 * words, dtype=I32))
    # a write through a view lands in the accumulator
    first = next(iter(want))
    v[first][(0,) * v[first].dim()] = 77
    assert int(acc[lay[first][0]]) == 77
    # refusals: short, not int64, not contiguous
    for bad in (acc[:-1], torch.zeros(words, dtype=F64), torch.zeros(words, dtype=I32), torch.zeros(2 * words, dtype=I64)[::2],
                acc.view(1, -1), acc.tolist()):
        with pytest.raises(ValueError, match="contiguous int64 vector"):
            views(bad)


def test_parameter_ranges_are_refused_by_family_name():
    for fn, bad, match in ((ops.eval_acc_layout, [(0, 4), (33, 4), (4, 6), (4, 0), (4, 1028)], "eval_acc"),
                           (ops.note_acc_layout, [(0,), (33,)], "note_stats"),
                           (ops.vae_eval_acc_layout, [(0, 8), (33, 8), (4, 0), (4, 1025)], "vae_eval_acc"),
                           (ops.cls_eval_layout, [(1, 15, 5), (17, 15, 5), (4, 0, 5), (4, 33, 5), (4, 15, 0), (4, 15, 65)],
                            "cls_eval_acc")):
        for args in bad:
            with pytest.raises(ValueError, match=match):
                fn(*args)


def test_packed_views_are_disjoint_typed_and_read_back_from_a_copy():
    parts = [("a", (3,), I64), ("b", (5,), F64), ("c", (3, 3), F32), ("d", (7,), I32), ("e", (2, 1, 3), F64), ("f", (1,), F32)]
    p = Packed(parts, "cpu")
    assert p.words == 3 + 5 + 5 + 4 + 6 + 1 and p.buf.dtype == I64 and tuple(p.buf.shape) == (p.words,)
    assert list(p.dev) == [n for n, _, _ in parts]
    spans, base = [], p.buf.data_ptr()
    for name, shape, dtype in parts:
        v = p.dev[name]
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous(), name
        lo = v.data_ptr() - base
        assert lo % 8 == 0 and 0 <= lo and lo + v.numel() * v.element_size() <= 8 * p.words
        spans.append((lo, lo + v.numel() * v.element_size()))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))            # in order, none overlaps the next
    g = torch.Generator().manual_seed(3)
    want = {}
    for name, shape, dtype in parts:
        want[name] = (torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g).to(dtype) if dtype in (I64, I32)
                      else torch.randn(shape, generator=g, dtype=dtype))
        p.dev[name].copy_(want[name])
    copy = p.buf.clone()                                                  # stands for the host copy of a device buffer
    p.buf.zero_()
    host = p.views(copy)
    for name, shape, dtype in parts:
        assert host[name].dtype == dtype and torch.equal(host[name], want[name]), name
        assert not p.dev[name].any()                                      # the first set follows its own buffer
    assert {k: tuple(v.shape) for k, v in p.host().items()} == {n: s for n, s, _ in parts}
    for bad in (copy[:-1], copy.to(F64), torch.zeros(2 * p.words, dtype=I64)[::2]):
        with pytest.raises(ValueError, match="Packed"):
            p.views(bad)
