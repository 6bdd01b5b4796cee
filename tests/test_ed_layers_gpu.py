"""emotion_discriminator/layers.py: the shared per-layer forward and backward of the classifier's MLP tail are the launches
they stand for -- the same ops.linear_fwd / ops.linear_dgrad / ops.linear_wgrad(defer=True) calls, in the same order, written
out here layer by layer -- so every output is compared with torch.equal: same launches, same bits.  5 and 7 rows (the batches
of the fixtures ed_latent_d8_b5 and ed_latent_d32_h3_b7) with two and three small hidden layers whose widths are no multiple of
a tile: the kernels' scalar and ragged paths and a last partial row group, where a wrong zout / emul / bias wiring would show.
ops.linear_* and ops.wgrad_multi refuse none of these widths."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {"b5_8_20_12_3": (5, (8, 20, 12, 3)), "b7_32_16_12_8_4": (7, (32, 16, 12, 8, 4))}


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


@pytest.fixture(scope="module")
def inputs():
    """Per case, made once and only read: the features, the layers' (weight, bias), the scaled keep-masks, dlogits."""
    out = {}
    for name, (rows, widths) in CASES.items():
        g = torch.Generator().manual_seed(len(widths))
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        layers = [((r(o, i) / i ** 0.5).cuda(), r(o).cuda()) for i, o in zip(widths[:-1], widths[1:])]
        masks = [((torch.rand(rows, h, generator=g) > 0.2).float() / 0.8).cuda() for h in widths[1:-1]]
        out[name] = (r(rows, widths[0]).cuda(), layers, masks, r(rows, widths[-1]).cuda())
    return out


class Bufs:
    """One run's outputs, full of NaN: an output a run does not write never compares equal."""

    def __init__(self, rows, widths, layers):
        nan = lambda *s: torch.full(s, float("nan"), device="cuda")      # noqa: E731
        hidden = widths[1:-1]
        self.cz, self.ca, self.dcz = ([nan(rows, h) for h in hidden] for _ in range(3))
        self.logits, self.dfeat = nan(rows, widths[-1]), nan(rows, widths[0])
        self.grads = [(nan(*w.shape), nan(*b.shape)) for w, b in layers]

    def tensors(self, wgrad, dfeat):
        t = self.cz + self.ca + self.dcz + [self.logits]
        return t + ([self.dfeat] if dfeat else []) + ([x for pair in self.grads for x in pair] if wgrad else [])


def written_out(ops, feat, layers, masks, dlogits, o, wgrad, dfeat):
    """The stack as individual launches: forward first to last, then from the head down -- each layer's weight-gradient job
    in front of its data-gradient launch, the first layer's last -- and one wgrad_multi over the jobs."""
    n = len(layers) - 1
    x = feat
    for j in range(n):
        w, b = layers[j]
        ops.linear_fwd(x, w, o.ca[j], bias=b, zout=o.cz[j], act=ops.ACT_GELU, emul=masks[j] if masks else None)
        x = o.ca[j]
    ops.linear_fwd(x, layers[n][0], o.logits, bias=layers[n][1])
    jobs, g = [], dlogits
    for j in range(n, 0, -1):          # layer j (n: the head) reads ca[j - 1]
        if wgrad:
            jobs.append(ops.linear_wgrad(o.ca[j - 1], g, o.grads[j][0], db=o.grads[j][1], defer=True))
        ops.linear_dgrad(g, layers[j][0], o.dcz[j - 1], gref=o.cz[j - 1], gact=ops.ACT_GELU, emul=masks[j - 1] if masks else None)
        g = o.dcz[j - 1]
    if wgrad:
        jobs.append(ops.linear_wgrad(feat, g, o.grads[0][0], db=o.grads[0][1], defer=True))
    if dfeat:
        ops.linear_dgrad(g, layers[0][0], o.dfeat)
    if wgrad:
        ops.wgrad_multi(jobs)
    return jobs


@pytest.mark.parametrize("dfeat", [False, True], ids=["no_dfeat", "dfeat"])
@pytest.mark.parametrize("wgrad", [False, True], ids=["no_wgrad", "wgrad"])
@pytest.mark.parametrize("masked", [False, True], ids=["no_masks", "masks"])
@pytest.mark.parametrize("case", list(CASES))
def test_tail_is_its_launches(ops, inputs, case, masked, wgrad, dfeat):
    from melo_gan_amd.emotion_discriminator.layers import tail_bwd, tail_fwd
    rows, widths = CASES[case]
    feat, layers, masks, dlogits = inputs[case]
    masks = masks if masked else None
    ref, got = Bufs(rows, widths, layers), Bufs(rows, widths, layers)
    ref_jobs = written_out(ops, feat, layers, masks, dlogits, ref, wgrad, dfeat)

    tail_fwd(feat, layers, got.cz, got.ca, got.logits, masks)
    jobs = [] if wgrad else None
    tail_bwd(dlogits, feat, layers, got.cz, got.ca, got.dcz, masks, got.dfeat if dfeat else None, jobs, got.grads if wgrad else None)
    if wgrad:
        # the job order is the launch's slice plan: head, hidden layers last to first, first layer
        assert [(j[9:], j[6].shape) for j in jobs] == [(j[9:], j[6].shape) for j in ref_jobs]
        assert [j[6] is got.grads[i][0] for j, i in zip(jobs, range(len(layers) - 1, -1, -1))] == [True] * len(layers)
        ops.wgrad_multi(jobs)
    torch.cuda.synchronize()
    for a, b in zip(got.tensors(wgrad, dfeat), ref.tensors(wgrad, dfeat)):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b)
    if not dfeat:
        assert torch.isnan(got.dfeat).all()          # no data-gradient launch for the first layer
