"""Synthetic PIV pairs on the device: particle images whose true displacement is a flow field you give -- a DNS field, a `.flo` an
earlier run wrote, an analytic vortex.  The package can score an estimate against a known field (`flow_errors`, `run.py --truth`);
this makes the pair to estimate from.  Under the reference's names (src/particle_image_generator.py: `ParticleImageGen`,
`random_particle`, `generate_image`, `create_pair_from_flow`), whose own version does not run.

Runs on csrc/particles.hip through the C ABI (`pivlfn_particles_displace`, `pivlfn_particles_render`; the arithmetic contract is
written out in include/pivlfn.h):

    gen = ParticleImageGen(density=0.05, seed=7)
    img1, img2, truth = gen.create_pair_from_flow(flow)        # flow [2,H,W] or [B,2,H,W] float32 on the device; uint8 images
    pos2, flag = displace_particles(pos, flow)                  # [2,N] float64 particles through one field
    frames = render_particles(pos, diam, amp, H, W)             # frames.image uint8, frames.intensity float32

The image model is the reference's: floor(density * area) particles seeded uniformly over the image and a margin of `pad` pixels round
it, diameter d = avg + std * U[0,1), grey level I = 240 exp(-z^2 / lt^2) for a particle at depth z in a light sheet of thickness lt,
every particle a Gaussian blob I exp(-r^2 / (d/2)^2).  A pixel adds its particles in ascending particle index, so an image has the same
bits alone, in any batch and from run to run.  Two deliberate departures from the reference:
  * pixel centres sit at integers from 0, as everywhere in this package (the reference's meshgrid starts at 1);
  * the grey level saturates at 255 (the reference's np.uint8(im) wraps round).
Seeding is host plumbing (a numpy Philox generator keyed by the seed, as in pivlfn.synth); moving and drawing the particles is on the
GPU.  GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _args, _lib

LOST, BAD = 2, 8                        # the bits of a particle's flag byte (PIVLFN_PARTICLES_*)
METHODS = {"bilinear": 0, "cubic": 1}
PEAK = 240.0                            # the grey level of a particle in the middle of the light sheet (the reference's)


class ParticleImages(NamedTuple):
    """What render_particles returns."""
    image: torch.Tensor           # uint8 [B,H,W] (or [H,W]): min(intensity, 255), truncated
    intensity: torch.Tensor       # float32, the same shape: the sum of the blobs before saturation


class PairParticles(NamedTuple):
    """The particles of B pairs as ParticleImageGen draws them: frame f of pair b is row f*B + b."""
    pos: torch.Tensor             # float64 [2B,2,N]
    diam: torch.Tensor            # float32 [2B,N]
    amp: torch.Tensor             # float32 [2B,N]
    flag: torch.Tensor            # uint8 [2B,N]: 0 in the first frames; LOST | BAD of the displacement in the second


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def check_method(method) -> int:
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"method={method!r} must be one of {', '.join(METHODS)}")
    return METHODS[method]


def check_image(H, W, radius=4, what="render_particles") -> None:
    """The size and radius checks of the renderer (ValueError / TypeError), usable before any tensor exists."""
    for name, v in (("H", H), ("W", W), ("radius", radius)):
        if not _args.is_integer(v):
            raise TypeError(f"{what}: {name}={v!r} must be an integer")
    if H < 1 or W < 1:
        raise ValueError(f"{what}: H={H} W={W} must both be positive")
    if H * W >= 1 << 31 or max(H, W) > (1 << 31) - 17:
        raise ValueError(f"{what}: H*W={H * W} pixels must stay below 2^31 and a side must not exceed 2^31 - 17")
    if not 1 <= radius <= 8:
        raise ValueError(f"{what}: radius={radius} must be 1..8 pixels")


def _check_tensor(t, name, dtype, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")


def _check_cuda(t, what):
    if not t.is_cuda:
        raise NotImplementedError(f"{what}: GPU tensors only")


def displace_particles(pos: torch.Tensor, flow: torch.Tensor, mask: Optional[torch.Tensor] = None, method: str = "bilinear",
                       flag: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Carries particles pos [2,N] float64 (x plane, y plane; pixel centres at integers) through the displacement field flow [2,H,W]
    float32: returns (pos + S(pos), flag) with S the bilinear or Catmull-Rom ("cubic") sample of the field at the position clamped to
    the image, so a particle in the margin round the image takes the edge's displacement.  `mask` [H,W] uint8 or bool: nonzero
    vectors are not to be used.  flag [N] uint8: LOST where a tap was masked or unknown (NaN, inf, 1e10), BAD where a coordinate was
    NaN; such a particle stays where it was.  `flag`: the flags on entry (default none set); a flagged particle is copied through.
    Enqueued on the current stream."""
    code = check_method(method)
    what = "displace_particles"
    _check_tensor(pos, "pos", torch.float64, what)
    _check_tensor(flow, "flow", torch.float32, what)
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool)):
        raise TypeError(f"{what}: expected a uint8 or bool mask [H,W], got {mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
    if flag is not None:
        _check_tensor(flag, "flag", torch.uint8, what)
    if pos.dim() != 2 or pos.size(0) != 2:
        raise ValueError(f"{what}: pos must be [2,N] (x plane, y plane), got {tuple(pos.shape)}")
    if flow.dim() != 3 or flow.size(0) != 2 or flow.size(1) < 2 or flow.size(2) < 2:
        raise ValueError(f"{what}: flow must be [2,H,W] with H, W >= 2, got {tuple(flow.shape)}")
    H, W, N = flow.size(1), flow.size(2), pos.size(1)
    if H * W >= 1 << 31 or N >= 1 << 31:
        raise ValueError(f"{what}: H*W={H * W} pixels and N={N} particles must both stay below 2^31")
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} does not belong to a field of {H} x {W}")
    if flag is not None and tuple(flag.shape) != (N,):
        raise ValueError(f"{what}: flag {tuple(flag.shape)} does not belong to {N} particles")
    _check_cuda(pos, what)
    for name, t in (("flow", flow), ("mask", mask), ("flag", flag)):
        if t is not None and t.device != pos.device:
            raise ValueError(f"{what}: {name} on {t.device}, pos on {pos.device}")
    pos, flow = pos.detach().contiguous(), flow.detach().contiguous()
    if mask is not None:
        mask = mask.detach().contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    oflag = flag.detach().clone() if flag is not None else torch.zeros([N], dtype=torch.uint8, device=pos.device)
    out = torch.empty_like(pos)
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().pivlfn_particles_displace(pos.data_ptr(), flow.data_ptr(), _args.ptr(mask), H, W, N, code, oflag.data_ptr(),
                                                         out.data_ptr(), _lib.stream_ptr(pos.device)), what)
    return out, oflag


def render_particles(pos: torch.Tensor, diam: torch.Tensor, amp: torch.Tensor, H: int, W: int, radius: int = 4,
                     flag: Optional[torch.Tensor] = None) -> ParticleImages:
    """Draws B images of N particles each: pos [B,2,N] float64, diam [B,N] float32 (diameter in pixels), amp [B,N] float32 (peak grey
    level); or one image from [2,N], [N], [N].  `flag` [B,N] uint8: a nonzero byte leaves the particle out, as do non-finite values,
    diam <= 0 and amp < 0.  A particle is drawn on the pixels within `radius` of floor(x), floor(y) (synth._render's footprint at 4).
    One call of pivlfn_particles_render for the whole batch, enqueued on the current stream."""
    what = "render_particles"
    check_image(H, W, radius, what)
    _check_tensor(pos, "pos", torch.float64, what)
    _check_tensor(diam, "diam", torch.float32, what)
    _check_tensor(amp, "amp", torch.float32, what)
    if flag is not None:
        _check_tensor(flag, "flag", torch.uint8, what)
    single = pos.dim() == 2
    if single:
        pos, diam, amp, flag = pos[None], diam[None], amp[None], (flag[None] if flag is not None else None)
    if pos.dim() != 3 or pos.size(1) != 2:
        raise ValueError(f"{what}: pos must be [B,2,N] or [2,N] (x plane, y plane), got {tuple(pos.shape[1:] if single else pos.shape)}")
    B, _, N = pos.shape
    for name, t in (("diam", diam), ("amp", amp), ("flag", flag)):
        if t is not None and tuple(t.shape) != (B, N):
            raise ValueError(f"{what}: {name} {tuple(t.shape[1:] if single else t.shape)} does not belong to pos "
                             f"{tuple(pos.shape[1:] if single else pos.shape)}")
    if N >= 1 << 31:
        raise ValueError(f"{what}: N={N} particles, must stay below 2^31")
    _check_cuda(pos, what)
    for name, t in (("diam", diam), ("amp", amp), ("flag", flag)):
        if t is not None and t.device != pos.device:
            raise ValueError(f"{what}: {name} on {t.device}, pos on {pos.device}")
    pos, diam, amp = pos.detach().contiguous(), diam.detach().contiguous(), amp.detach().contiguous()
    flag = flag.detach().contiguous() if flag is not None else None
    lib = _lib.load()
    intensity = torch.empty([B, H, W], dtype=torch.float32, device=pos.device)
    image = torch.empty([B, H, W], dtype=torch.uint8, device=pos.device)
    ws = torch.empty(lib.pivlfn_particles_render_workspace_bytes(B, N, H, W, radius), dtype=torch.uint8, device=pos.device)
    with torch.cuda.device(pos.device):
        _lib.check(lib.pivlfn_particles_render(pos.data_ptr(), diam.data_ptr(), amp.data_ptr(), _args.ptr(flag), B, N, H, W, radius,
                                               intensity.data_ptr(), image.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(pos.device)), what)
    return ParticleImages(image[0], intensity[0]) if single else ParticleImages(image, intensity)


class ParticleImageGen:
    """The reference's particle-image generator (src/particle_image_generator.py:9-20) with its constructor names and their meaning:
    `density` particles per pixel, diameter avg_diameter + std_diameter * U[0,1) pixels, grey level 240 exp(-z^2 / laser_thickness^2)
    with the depth z uniform in [-0.5, 0.5).  `seed` keys the generator: the same seed gives the same particles on every machine."""

    def __init__(self, density: float = 0.05, avg_diameter: float = 1.5, std_diameter: float = 1, laser_thickness: float = 1,
                 seed: int = 0, device="cuda"):
        for name, v in (("density", density), ("avg_diameter", avg_diameter), ("std_diameter", std_diameter),
                        ("laser_thickness", laser_thickness)):
            if not _is_real(v):
                raise TypeError(f"ParticleImageGen: {name}={v!r} must be a number")
            if not math.isfinite(v) or v < 0:
                raise ValueError(f"ParticleImageGen: {name}={v!r} must be finite and not negative")
        if avg_diameter + std_diameter <= 0:
            raise ValueError("ParticleImageGen: avg_diameter and std_diameter are both 0: the particles would have no size")
        if laser_thickness <= 0:
            raise ValueError(f"ParticleImageGen: laser_thickness={laser_thickness!r} must be positive")
        if not _args.is_integer(seed):
            raise TypeError(f"ParticleImageGen: seed={seed!r} must be an integer")
        self.p_density, self.p_avg_d, self.p_std_d, self.lt = float(density), float(avg_diameter), float(std_diameter), float(laser_thickness)
        self.seed = int(seed)
        self.device = torch.device(device)

    # ---- host plumbing: the seeding ---------------------------------------------------------------------------------------------------
    def count(self, H: int, W: int, pad: int = 0) -> int:
        """floor(density * area) over the padded area, as the reference counts."""
        check_image(H, W, 4, "ParticleImageGen")
        if not _args.is_integer(pad):
            raise TypeError(f"ParticleImageGen: pad={pad!r} must be an integer")
        if not 0 <= pad <= 1 << 20:
            raise ValueError(f"ParticleImageGen: pad={pad} must be 0..2^20 pixels")
        n = int(math.floor(self.p_density * (H + 2 * pad) * (W + 2 * pad)))
        if n >= 1 << 31:
            raise ValueError(f"ParticleImageGen: {n} particles, must stay below 2^31")
        return n

    def _seeding(self, H, W, pad, seed, out_of_plane=0.0):
        """numpy float64 x, y, z, d and the depth in the second frame, drawn in this order from one Philox generator keyed by seed."""
        n = self.count(H, W, pad)
        g = np.random.Generator(np.random.Philox(key=[seed & 0xFFFFFFFF, 0x50495647]))
        x = g.random(n) * (W + 2 * pad) - pad
        y = g.random(n) * (H + 2 * pad) - pad
        z = g.random(n) - 0.5
        d = self.p_avg_d + self.p_std_d * g.random(n)
        z2 = z + out_of_plane * g.standard_normal(n) if out_of_plane else z
        return x, y, z, d, z2

    def random_particle(self, H: int, W: int, pad: int = 0):
        """The seeding of one image: device tensors x, y, z (float64) and d (float32), count(H, W, pad) of each, x in [-pad, W + pad)
        and y in [-pad, H + pad)."""
        x, y, z, d, _ = self._seeding(H, W, pad, self.seed)
        dev = self._device()
        return (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(z).to(dev),
                torch.from_numpy(d.astype(np.float32)).to(dev))

    def _device(self):
        if self.device.type != "cuda":
            raise NotImplementedError("ParticleImageGen: GPU only")
        return self.device

    def amplitude(self, z: torch.Tensor) -> torch.Tensor:
        """The peak grey level 240 exp(-z^2 / lt^2) of particles at depth z, formed in float64 and rounded to float32."""
        z = z.to(torch.float64)
        return (PEAK * torch.exp(-(z * z) / (self.lt * self.lt))).to(torch.float32)

    # ---- the device side --------------------------------------------------------------------------------------------------------------
    def generate_image(self, x: torch.Tensor, y: torch.Tensor, z: torch.Tensor, d: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """The uint8 [H,W] image of the particles (x, y, z, d) -- device tensors, as random_particle returns them."""
        check_image(H, W, 4, "generate_image")
        for name, t in (("x", x), ("y", y), ("z", z), ("d", d)):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.dim() != 1 or t.numel() != x.numel():
                raise TypeError(f"generate_image: {name} must be a floating-point tensor [N] like x")
        pos = torch.stack([x.to(torch.float64), y.to(torch.float64)])
        return render_particles(pos, d.to(torch.float32), self.amplitude(z), H, W).image

    def pair_particles(self, flow: torch.Tensor, pad: int = 16, method: str = "cubic", mask: Optional[torch.Tensor] = None,
                       out_of_plane: float = 0.0) -> PairParticles:
        """The particles create_pair_from_flow draws, for flows [B,2,H,W]: pair b is seeded from seed + b and displaced by flow b."""
        code_checked = check_method(method)                         # noqa: F841  (every parameter check comes before any tensor)
        if not _is_real(out_of_plane):
            raise TypeError(f"create_pair_from_flow: out_of_plane={out_of_plane!r} must be a number")
        if not math.isfinite(out_of_plane) or out_of_plane < 0:
            raise ValueError(f"create_pair_from_flow: out_of_plane={out_of_plane!r} must be finite and not negative")
        if not _args.is_integer(pad):
            raise TypeError(f"create_pair_from_flow: pad={pad!r} must be an integer")
        if not 0 <= pad <= 1 << 20:
            raise ValueError(f"create_pair_from_flow: pad={pad} must be 0..2^20 pixels")
        _check_tensor(flow, "flow", torch.float32, "create_pair_from_flow")
        if flow.dim() != 4 or flow.size(1) != 2:
            raise ValueError(f"create_pair_from_flow: expected flows [B,2,H,W], got {tuple(flow.shape)}")
        B, _, H, W = flow.shape
        if mask is not None and (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, H, W)):
            raise ValueError(f"create_pair_from_flow: the mask must be a tensor [B,H,W] = {(B, H, W)}")
        _check_cuda(flow, "create_pair_from_flow")
        dev = flow.device
        N = self.count(H, W, pad)
        pos = torch.empty([2, B, 2, N], dtype=torch.float64, device=dev)
        diam = torch.empty([2, B, N], dtype=torch.float32, device=dev)
        amp = torch.empty([2, B, N], dtype=torch.float32, device=dev)
        flag = torch.zeros([2, B, N], dtype=torch.uint8, device=dev)
        for b in range(B):
            x, y, z, d, z2 = self._seeding(H, W, pad, self.seed + b, float(out_of_plane))
            pos[0, b].copy_(torch.from_numpy(np.stack([x, y])), non_blocking=False)
            diam[:, b] = torch.from_numpy(d.astype(np.float32)).to(dev)
            amp[0, b] = self.amplitude(torch.from_numpy(z).to(dev))
            amp[1, b] = self.amplitude(torch.from_numpy(z2).to(dev))
            pos[1, b], flag[1, b] = displace_particles(pos[0, b], flow[b], mask[b] if mask is not None else None, method)
        return PairParticles(pos.view(2 * B, 2, N), diam.view(2 * B, N), amp.view(2 * B, N), flag.view(2 * B, N))

    def create_pair_from_flow(self, flow: torch.Tensor, pad: int = 16, method: str = "cubic", mask: Optional[torch.Tensor] = None,
                              out_of_plane: float = 0.0):
        """An image pair (or B pairs) whose true displacement is `flow`: [2,H,W] or [B,2,H,W] float32 on the device.  Returns
        (img1, img2, truth): uint8 [B,H,W] images ([H,W] for one flow) and the flow as it was given.

        Particles are seeded over the image and `pad` pixels round it (pair b from seed + b), drawn, carried through the flow by
        displace_particles (`method` "cubic" or "bilinear"; `mask` [B,H,W] or [H,W], nonzero = unknown vector) and drawn again; both
        frames of all pairs are one render launch.  `out_of_plane` is the standard deviation of a depth change between the frames:
        frame 2 uses z + out_of_plane * N(0,1) from the same seeded generator, so the particles' brightness differs.
        A particle that meets a masked or unknown vector (LOST) is drawn in frame 1 and left out of frame 2: it has no known
        displacement, and the pixels under it are the ones the truth says nothing about."""
        single = isinstance(flow, torch.Tensor) and flow.dim() == 3
        if single:
            flow4, mask = flow[None], (mask[None] if isinstance(mask, torch.Tensor) else mask)
        else:
            flow4 = flow
        p = self.pair_particles(flow4, pad, method, mask, out_of_plane)
        B, H, W = flow4.size(0), flow4.size(2), flow4.size(3)
        image = render_particles(p.pos, p.diam, p.amp, H, W, 4, p.flag).image.view(2, B, H, W)
        return (image[0, 0], image[1, 0], flow) if single else (image[0], image[1], flow)
