"""The reference's import path for its error measures (src/loss.py), for evaluation: EPE, L1, L2, L1Loss, L2Loss, MultiScale,
LevelLoss, hui_loss and piv_loss with the reference's signatures, defaults, pool sizes, weights and return shapes, computed on the
device by pivlfn.evaluate (csrc/evaluate.hip).

Evaluation only -- there is no training here: every result is a 0-dim float64 tensor on the flows' device without a graph.  A mean over
a batch is formed from the per-pair float64 sums, added in pair order.  Pixels whose truth is unknown (NaN or beyond 1e9) are left out
of sums and counts; with a fully known truth the values are the reference's up to float64 rounding.  A pooled window must be a power
of two up to 32: startScale 1 or 2 with the usual levels.  piv_loss(level_eval=True, version=2) asks for a 64 x 64 window at its
first level and is refused."""
from typing import List, Tuple, Union

import torch

from pivlfn.evaluate import flow_errors

__all__ = ['hui_loss', 'piv_loss']

HUI_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)
PIV_WEIGHTS = {1: (0.001, 0.001, 0.001, 0.001, 0.001, 0.01), 2: (0.001, 0.001, 0.001, 0.001, 0.01)}     # Cai et al. 2019


def _seq(t: torch.Tensor) -> torch.Tensor:
    """The entries of a [B] tensor added in order."""
    s = t[0]
    for i in range(1, t.numel()):
        s = s + t[i]
    return s


def _score(output, target, pool=1, div_flow=1.0):
    if pool < 1 or pool & (pool - 1) or pool > 32:
        raise ValueError(f'pooled window {pool} is not a power of two up to 32 (startScale * 2**scale)')
    if output.size(0) == 0:
        raise ValueError('an empty batch has no error')
    return flow_errors(output, target, pool=pool, div_flow=div_flow)


def _epe(err, mean):
    return _seq(err.epe) / _seq(err.n) if mean else _seq(err.epe) / err.epe.numel()


def _l1(err, mean):
    return _seq(err.l1) / (2.0 * _seq(err.n)) if mean else _seq(err.l1) / err.l1.numel()


def _windows(start, count):
    """Pooled window sizes of `count` pyramid levels, coarsest first, the finest one `start` pixels wide."""
    return [start * 2 ** k for k in range(count - 1, -1, -1)]


def _as_list(level):
    return list(level) if type(level) in (tuple, list) else [level]


def EPE(input_flow, target_flow, mean=True):
    """Mean end-point error over all pixels (mean=True) or its sum per pair (mean=False)."""
    return _epe(_score(input_flow, target_flow), mean)


class _Norm(torch.nn.Module):
    def __init__(self, mean=True):
        super().__init__()
        self.mean = mean

    def forward(self, output, target):
        return self.of(_score(output, target))


class L1(_Norm):
    """|du| + |dv| averaged over pixels and both components (mean=True) or summed per pair."""
    def __init__(self, mean=True):
        super().__init__(mean)

    def of(self, err):
        return _l1(err, self.mean)


class L2(_Norm):
    """The per-pixel 2-norm of the difference, i.e. the end-point error, averaged or summed like L1."""
    def __init__(self, mean=True):
        super().__init__(mean)

    def of(self, err):
        return _epe(err, self.mean)


class _Scaled(torch.nn.Module):
    def forward(self, output, target):
        err = _score(output, target)
        return [self.mul_flow * self.loss.of(err), self.mul_flow * _epe(err, True)]


class L1Loss(_Scaled):
    def __init__(self, mul_scale=1):
        super().__init__()
        self.mul_flow, self.loss, self.loss_labels = float(mul_scale), L1(), ['L1', 'EPE']


class L2Loss(_Scaled):
    def __init__(self, mul_scale=1):
        super().__init__()
        self.mul_flow, self.loss, self.loss_labels = float(mul_scale), L2(), ['L2', 'EPE']


class MultiScale(torch.nn.Module):
    """Weighted error over the pyramid (levels coarsest first: 6, 5, ...), or, for a single flow, the error at the lowest level.
    div_scale: what the truth is multiplied by in the per-level branch; startScale: the lowest level, i.e. the smallest pooled
    window; l_weight: one weight per entry of the per-level list; norm: 'L1' or 'L2'.  The defaults are LiteFlowNet's (Hui 2018)."""
    def __init__(self, div_scale: float = 0.05, startScale: int = 2, use_mean: bool = True,
                 l_weight: Union[Tuple[float, ...], List[float]] = (0.32, 0.08, 0.02, 0.01, 0.005), norm: str = 'L1'
                 ) -> None:
        super().__init__()
        if not isinstance(l_weight, (list, tuple)):
            raise ValueError(f'l_weight must be a list or tuple of per-level weights, got {l_weight!r}')
        if norm not in ('L1', 'L2'):
            raise ValueError(f"norm must be 'L1' or 'L2', got {norm!r}")
        self.loss_weights, self.use_mean, self.div_flow = l_weight, use_mean, div_scale
        self.startScale, self.numScales = startScale, 7 - startScale
        self.multiScales = _windows(startScale, self.numScales)
        self.loss = (L1 if norm == 'L1' else L2)(mean=use_mean)
        self.loss_labels = ['MultiScale-' + norm, 'EPE'],

    def forward(self, output: Union[torch.Tensor, List[torch.Tensor]], target: torch.Tensor):
        if type(output) not in (tuple, list):
            # one flow: the lowest level against the pooled truth as it is (no div_flow), as the reference evaluates
            err = _score(output, target, self.multiScales[-1])
            return [0.0 + self.loss.of(err), 0.0 + _epe(err, self.use_mean)]
        assert len(self.loss_weights) == len(output)
        lossvalue, epevalue = 0.0, 0.0
        for i, level in enumerate(output):
            pool = self.multiScales[i] if i < self.numScales else 1
            for flow in _as_list(level):
                err = _score(flow, target, pool, self.div_flow)
                epevalue = epevalue + self.loss_weights[i] * _epe(err, self.use_mean)
                lossvalue = lossvalue + self.loss_weights[i] * self.loss.of(err)
        return [lossvalue, epevalue]


class LevelLoss(torch.nn.Module):
    """The error of every pyramid level on its own (levels coarsest first); of a level given as a list, its last flow counts."""
    def __init__(self, div_scale: float = 0.05, startScale: int = 2, n_level: int = 5, norm: str = 'L1') -> None:
        super().__init__()
        self.startScale, self.numScales, self.div_flow = startScale, n_level, div_scale
        self.multiScales = _windows(startScale, n_level)
        self.loss = L1() if norm == 'L1' else L2()
        self.loss_labels = ['MultiScale-' + norm, 'EPE'],

    def forward(self, output, target):
        if type(output) not in (tuple, list):
            raise ValueError('per-level evaluation needs a list or tuple of per-level flows')
        assert self.numScales == len(output)
        lossvalue, epevalue = [], []
        for level, pool in zip(output, self.multiScales):
            err = _score(_as_list(level)[-1], target, pool, self.div_flow)
            epevalue.append(_epe(err, True))
            lossvalue.append(self.loss.of(err))
        return [lossvalue, epevalue]


def hui_loss(level_eval=False, mul_scale=20, norm='L1'):
    """LiteFlowNet's measure: the per-level table (level_eval) or the weighted total."""
    cls = LevelLoss if level_eval else MultiScale
    return cls(div_scale=1/mul_scale, norm=norm)


def piv_loss(level_eval=False, mul_scale=5, norm='L1', version: int = 1):
    """PIV-LiteFlowNet-en's (version 1, six levels down to full resolution) and PIV-LiteFlowNet2-en's (version 2) measure."""
    if version not in PIV_WEIGHTS:
        raise ValueError(f'version must be 1 or 2, got {version!r}')
    if level_eval:
        return LevelLoss(div_scale=1 / mul_scale, startScale=version, n_level=6, norm=norm)
    return MultiScale(div_scale=1 / mul_scale, startScale=version, l_weight=PIV_WEIGHTS[version], norm=norm)
