"""The refusals and the files of the streaming accumulators (FlowStats, MaskedFlowStats, ErrorStats, UncertaintyStats, TwoPointStats,
FlowDistribution, FrameBackground, TemporalSpectrum, PressureField, FlowPOD, FlowMap), case by case.  A helper, not a test:
tools/gen_accumulator_golden.py records what the cases below give into tests/golden/accumulator_refusals.json, and
tests/test_accumulators.py and tests/test_gpu_accumulators.py replay them and compare for equality.

Three parts.  `constructor_cases()`: the constructor refusals that need no GPU (a size of 0 x 9 and of 8 x 0, device="cpu", 16385
columns for TwoPointStats).  `update_cases(dev)`: with accumulators of 8 x 9 on `dev`, frames of 8 x 10, a mask of another shape where
the class takes one, and a `mean` or `scale` of another shape where the constructor takes one; none of them launches anything.
`save_members(dev, tmp)`: the member names, dtypes and shapes of every save() file after one update() of two frames.  The texts of the
second part name the device, so `dev` is always an indexed one."""
import os

H, W, B = 8, 9, 2
SIZED = ("FlowStats", "MaskedFlowStats", "ErrorStats", "UncertaintyStats", "TwoPointStats", "FlowDistribution", "FrameBackground")
OTHERS = ("TemporalSpectrum", "PressureField", "FlowPOD", "FlowMap")
SAVED = SIZED[:6] + ("TemporalSpectrum",)                       # FrameBackground.save writes a picture


def make(name, h=H, w=W, device="cuda:0", **kw):
    """One accumulator of the class `name`, with small parameters where the class has some."""
    import pivlfn
    from pivlfn.postpro import FlowStats
    if name in ("FlowStats", "MaskedFlowStats"):
        return (FlowStats if name == "FlowStats" else pivlfn.MaskedFlowStats)(h, w, 1.0, device)
    if name == "TwoPointStats":
        return pivlfn.TwoPointStats(h, w, max_sep=3, device=device, **kw)
    if name == "FlowDistribution":
        return pivlfn.FlowDistribution(h, w, bins=16, joint_bins=4, frac_bins=4, device=device, **kw)
    if name == "TemporalSpectrum":
        return pivlfn.TemporalSpectrum(h, w, segment=2, device=device)
    if name == "PressureField":
        return pivlfn.PressureField(h, w, cell=4, device=device)
    if name == "FlowPOD":
        return pivlfn.FlowPOD(h, w, 4, device=device)
    return getattr(pivlfn, name)(h, w, device=device)              # ErrorStats, UncertaintyStats, FrameBackground, FlowMap


def frames(name, dev, h=H, w=W, mask_w=None, seed=0):
    """The arguments of `name`.update for B frames of h x w on `dev`; with `mask_w` the mask (flag) is [B,h,mask_w] instead."""
    import torch
    import pivlfn
    g = torch.Generator().manual_seed(seed)
    flow = torch.randn(B, 2, h, w, generator=g).to(dev)
    mask = (torch.rand(B, h, mask_w or w, generator=g) < 0.25).to(torch.uint8).to(dev)
    if name == "FrameBackground":
        return (torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8).to(dev),)
    if name == "UncertaintyStats":
        return (pivlfn.FlowUncertainty(flow.abs(), mask),)
    if name == "ErrorStats":
        return (flow, torch.randn(B, 2, h, w, generator=g).to(dev)) + ((mask,) if mask_w else ())
    if name == "MaskedFlowStats":
        return (flow, mask)
    return (flow, mask) if mask_w else (flow,)


def outcome(fn):
    """What `fn()` raises, as {"type", "text"}; None if it raises nothing."""
    try:
        fn()
    except Exception as e:                                          # noqa: BLE001  (whatever it is gets recorded)
        return {"type": type(e).__name__, "text": str(e)}
    return None


def constructor_cases():
    import pivlfn
    out = {}
    for name in SIZED + OTHERS:
        out[f"{name} 0x9"] = outcome(lambda: make(name, 0, 9))
        out[f"{name} 8x0"] = outcome(lambda: make(name, 8, 0))
        if name != "FlowPOD":                                       # FlowPOD takes a store on the host and refuses at update()
            out[f"{name} cpu"] = outcome(lambda: make(name, device="cpu"))
    out["TwoPointStats 8x16385"] = outcome(lambda: make("TwoPointStats", 8, 16385))
    out["color_wheel_image cpu"] = outcome(lambda: pivlfn.color_wheel_image(5, device="cpu"))
    return out


def update_cases(dev):
    import numpy as np
    out = {}
    for name in SIZED + OTHERS:
        acc = make(name, device=dev)
        out[f"{name} frames 8x10"] = outcome(lambda: acc.update(*frames(name, dev, w=W + 1)))
        if name not in ("FlowStats", "FrameBackground"):            # these two take no mask
            out[f"{name} mask 8x10"] = outcome(lambda: acc.update(*frames(name, dev, mask_w=W + 1)))
    wrong = np.zeros((2, H, W + 1))
    out["TwoPointStats mean 8x10"] = outcome(lambda: make("TwoPointStats", device=dev, mean=wrong))
    out["FlowDistribution mean 8x10"] = outcome(lambda: make("FlowDistribution", device=dev, mean=wrong))
    out["FlowDistribution scale 8x10"] = outcome(lambda: make("FlowDistribution", device=dev, scale=wrong))
    return out


def save_members(dev, tmp):
    import numpy as np
    out = {}
    for name in SAVED:
        acc = make(name, device=dev)
        acc.update(*frames(name, dev))
        path = acc.save(os.path.join(str(tmp), name))               # no suffix given: save() adds it and returns the path
        with np.load(path) as f:
            out[name] = {"file": os.path.basename(path), "members": {k: [str(f[k].dtype), list(f[k].shape)] for k in f.files}}
    return out
