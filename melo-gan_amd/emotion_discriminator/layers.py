"""The emotion classifier's MLP tail -- (Linear, GELU[, Dropout])* and the head (ed_model.py:72-95) -- as per-layer launches,
written once: the training engines (EdEngine, EdLatentEngine's comparator) and the frozen classifier of GanEngine call these.

`layers` is the tail's [(weight, bias)] in forward order, the head last; cz / ca / dcz hold one tensor per hidden layer;
`masks` the hidden layers' dropout keep-masks (scaled), None in eval mode and for the frozen classifier.
"""
from .. import ops
from ..ops import ACT_GELU


def tail_fwd(feat, layers, cz, ca, logits, masks=None):
    """feat -> logits; hidden layer j leaves its pre-activation in cz[j] and GELU (times masks[j]) in ca[j]."""
    for j, (w, b) in enumerate(layers[:-1]):
        ops.linear_fwd(feat, w, ca[j], bias=b, zout=cz[j], act=ACT_GELU, emul=masks[j] if masks else None)
        feat = ca[j]
    ops.linear_fwd(feat, layers[-1][0], logits, bias=layers[-1][1])


def tail_bwd(dlogits, feat, layers, cz, ca, dcz, masks=None, dfeat=None, jobs=None, grads=None):
    """dlogits back through the tail, last layer first: the gradient reaching hidden layer j's pre-activation -- times
    GELU'(cz[j]) and masks[j] -- into dcz[j], and the gradient of `feat` into dfeat where one is given.  jobs: a list that
    receives each layer's deferred weight-gradient job (into grads, [(dW, db)] like `layers`) in front of that layer's
    data-gradient launch; the caller launches them (ops.wgrad_multi) with its others."""
    g = dlogits
    for j in range(len(layers) - 1, -1, -1):
        if jobs is not None:
            jobs.append(ops.linear_wgrad(ca[j - 1] if j else feat, g, grads[j][0], db=grads[j][1], defer=True))
        if j:
            ops.linear_dgrad(g, layers[j][0], dcz[j - 1], gref=cz[j - 1], gact=ACT_GELU, emul=masks[j - 1] if masks else None)
            g = dcz[j - 1]
        elif dfeat is not None:
            ops.linear_dgrad(g, layers[0][0], dfeat)
