"""Exponential moving average of the generator's weights (Yazici et al. 2019, "The unusual effectiveness of averaging in GAN training"): the config keys, the decay schedule
and the host restatement of mg_ema_flat (csrc/ema.hip) that the tests hold the kernel to, bit for bit.  Host code only: numpy,
no GPU import.

    EMA_DECAY   0 (default) = off; 0 < d < 1 keeps an fp64 shadow of G and E_num, updated behind every generator update
    EMA_RAMP    true (default): update t (counted from 0 where averaging began) uses min(d, (1 + t) / (10 + t))
"""
from __future__ import annotations

from typing import Sequence, Tuple, Union

import numpy as np

RAMP_NUM, RAMP_DEN = 1.0, 10.0


def ema_config(cfg: dict) -> Tuple[float, bool]:
    """(EMA_DECAY, EMA_RAMP) of a GAN config; both keys are optional.  ValueError unless 0 <= EMA_DECAY < 1."""
    raw = cfg.get("EMA_DECAY", 0.0)
    if isinstance(raw, (bool, str)) or not isinstance(raw, (int, float, np.integer, np.floating)):
        raise ValueError(f"EMA_DECAY = {raw!r}: a number in [0, 1) expected (0 = off)")
    d = float(raw)
    if not 0.0 <= d < 1.0:            # false for a NaN too
        raise ValueError(f"EMA_DECAY = {raw!r}: must be in [0, 1) (0 = off)")
    ramp = cfg.get("EMA_RAMP", True)
    if not isinstance(ramp, (bool, np.bool_)):
        raise ValueError(f"EMA_RAMP = {ramp!r}: true or false expected")
    return d, bool(ramp)


def ema_decay_at(t: float, decay: float, ramp: bool) -> float:
    """The decay of the update that has t averaged updates before it: fp64, one IEEE divide, as the kernel."""
    decay = np.float64(decay)
    if not ramp:
        return decay
    t = np.float64(t)
    r = (np.float64(RAMP_NUM) + t) / (np.float64(RAMP_DEN) + t)
    return r if r < decay else decay


def ema_ref(p_list: Sequence[np.ndarray], decay: float, ramp: bool, offset: float, step0: Union[int, Sequence[int]], *,
            shadow0: np.ndarray) -> np.ndarray:
    """The shadow after one mg_ema_flat launch per entry of p_list, starting from shadow0 (fp64; not modified).

    p_list[k]: the fp32 parameters as update k left them.  step0: the optimiser's step count when the first launch runs (that
    update included) -- later launches see step0 + k -- or the list of the step counts of every launch.  offset: the step count
    at which averaging began.  Per element, every operation rounded on its own:
        s = s + (1 - d) * (float64(p) - s),   d = ema_decay_at(step - 1 - offset, decay, ramp)."""
    steps = [int(step0) + k for k in range(len(p_list))] if np.isscalar(step0) else [int(s) for s in step0]
    if len(steps) != len(p_list):
        raise ValueError("ema_ref: one step count per entry of p_list")
    s = np.array(shadow0, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):     # non-finite parameters propagate, as on the device
        for p, step in zip(p_list, steps):
            p = np.asarray(p)
            if p.dtype != np.float32 or p.shape != s.shape:
                raise ValueError("ema_ref: fp32 parameters of the shadow's shape expected")
            t = (np.float64(step) - np.float64(1.0)) - np.float64(offset)
            omd = np.float64(1.0) - ema_decay_at(t, decay, ramp)
            diff = p.astype(np.float64) - s
            inc = omd * diff
            s = s + inc
    return s
