"""Snapshot POD of a flow sequence: which coherent structures carry the fluctuation energy.

The method of snapshots: the n flows of a sequence are rows of X [n,P]; the eigenvectors of the centred Gram matrix C = J X X^T J
(J = I - 11^T/n) give the temporal coefficients, and the spatial modes are weighted sums of the snapshots.  The two heavy steps run
in libpivlfn.so -- the Gram matrix in fp64 on the fp64 matrix instruction (pivlfn_snapshot_gram) and the weighted sums
(pivlfn_snapshot_project) -- the n x n eigenproblem is numpy.linalg.eigh on the host.

    pod = FlowPOD(H, W, capacity=n_pairs, cell=4)
    for flows in batches:
        pod.update(flows)                # never synchronises; with validate_flow's flag bytes as mask= where vectors were rejected
    res = pod.solve(modes=8)             # PODResult: modes, mean, coeff, energy, fraction, eigenvalues, gram
    res.save("pod.npz")
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _accum, _args, _lib

MAX_SNAPSHOTS = 4096          # PIVLFN_POD_MAX_SNAPSHOTS
MAX_MODES = 64
DEGENERATE = 1e-12            # a mode with eigenvalue <= DEGENERATE * max(the largest, trace(G)) is undefined


@dataclass
class PODResult:
    """All NumPy float64.  modes [K,2,ch,cw], orthonormal over the grid;  mean [2,ch,cw];  coeff [n,K], snapshot i is
    mean + sum_k coeff[i,k] * modes[k] (exactly, with K = rank);  energy [K] = eigenvalue / n, the mean squared fluctuation carried by
    the mode;  fraction [K] of the total fluctuation energy;  eigenvalues [n] of the centred Gram matrix, descending;  gram [n,n]."""
    modes: np.ndarray
    mean: np.ndarray
    coeff: np.ndarray
    energy: np.ndarray
    fraction: np.ndarray
    eigenvalues: np.ndarray
    gram: np.ndarray
    cell: int
    H: int
    W: int

    def reconstruct(self, i: int, r: Optional[int] = None) -> np.ndarray:
        """Snapshot i from the mean and its first r modes (all kept modes by default): [2,ch,cw]."""
        K = self.modes.shape[0]
        r = K if r is None else r
        if not _args.is_integer(r) or not 0 <= r <= K:
            raise ValueError(f"reconstruct: r={r!r} must be 0..{K}, the modes kept")
        if not -self.coeff.shape[0] <= i < self.coeff.shape[0]:
            raise IndexError(f"reconstruct: snapshot {i} of {self.coeff.shape[0]}")
        return self.mean + np.tensordot(self.coeff[i, :r], self.modes[:r], axes=1)

    def save(self, path: str) -> str:
        np.savez(path, modes=self.modes, mean=self.mean, coeff=self.coeff, energy=self.energy, fraction=self.fraction,
                 eigenvalues=self.eigenvalues, gram=self.gram, cell=np.int64(self.cell), H=np.int64(self.H), W=np.int64(self.W))
        return path


def check_capacity(capacity) -> int:
    if not _args.is_int(capacity, 2, MAX_SNAPSHOTS):
        raise ValueError(f"FlowPOD: capacity={capacity!r} must be an integer from 2 to {MAX_SNAPSHOTS} snapshots (the Gram matrix is "
                         "solved on the host)")
    return capacity


def check_solve(n: int, modes, empty: int) -> int:
    """The refusals of FlowPOD.solve that need no arithmetic."""
    if empty != 0:
        raise ValueError(f"FlowPOD.solve: {empty} cells of the stored snapshots are empty (every vector in them unknown or masked); POD "
                         "has no value to put there: fill them first (run.py --validate replace) or average over a larger cell")
    if n < 2:
        raise ValueError(f"FlowPOD.solve: {n} snapshot(s) stored, at least 2 are needed")
    top = min(MAX_MODES, n - 1)
    if not _args.is_int(modes, 1, top):
        raise ValueError(f"FlowPOD.solve: modes={modes!r} must be 1..{top} (at most {MAX_MODES}, and n - 1 = {n - 1}: centring takes one "
                         "degree of freedom)")
    return modes


def sign_rule(V: np.ndarray) -> np.ndarray:
    """A copy of V [n,K] with the entry of largest magnitude of every column made positive; of equal entries the first decides."""
    V = np.array(V, dtype=np.float64)
    top = np.abs(V).argmax(axis=0)                      # argmax returns the first of equal entries
    V *= np.where(V[top, np.arange(V.shape[1])] < 0, -1.0, 1.0)
    return V


def solve_gram(G: np.ndarray, K: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host half of the method of snapshots.  G [n,n] float64 -> (eigenvalues [n] of J G J descending, V [n,K] the first K
    eigenvectors with the entry of largest magnitude of each made positive (the first such entry on a tie), Wt [n,K+1] =
    [J V diag(lambda)^-1/2 | 1], the weights whose sums over the snapshots are the spatial modes and n times the mean)."""
    n = G.shape[0]
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    C = J @ G @ J
    lam, V = np.linalg.eigh(C)
    lam, V = lam[::-1].copy(), V[:, ::-1]
    # trace(G) stands beside lambda_1 because J G J of snapshots that do not fluctuate at all is not 0 but the rounding of the
    # centring, a few ulp of trace(G): without it n identical snapshots would pass with a "largest" eigenvalue of pure noise
    floor = DEGENERATE * max(lam[0], np.trace(G))
    for k in range(K):
        if not lam[k] > floor:
            raise ValueError(f"FlowPOD.solve: mode {k + 1} is undefined: its eigenvalue {lam[k]:.3e} is not above {DEGENERATE:g} of the "
                             f"largest ({lam[0]:.3e}) or of the snapshots' total energy ({np.trace(G):.3e}); the snapshots span fewer "
                             f"than {k + 1} directions around their mean")
    V = sign_rule(V[:, :K])
    Wt = np.concatenate([(J @ V) / np.sqrt(lam[:K]), np.ones((n, 1))], axis=1)
    return lam, V, np.ascontiguousarray(Wt)


def snapshot_gram(X: torch.Tensor, n: int, P: int) -> torch.Tensor:
    """G [n,n] float64 on X's device from the first n rows and P columns of X (float32, 2-D, unit column stride)."""
    if X.dim() != 2 or X.dtype != torch.float32 or not X.is_cuda or X.stride(1) != 1 or X.size(0) < n or X.size(1) < P:
        raise ValueError("snapshot_gram: X must be a float32 [rows >= n, columns >= P] device tensor with unit column stride")
    lib = _lib.load()
    G = torch.empty([n, n], dtype=torch.float64, device=X.device)
    nbytes = lib.pivlfn_snapshot_gram_workspace_bytes(n, P)
    ws = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(lib.pivlfn_snapshot_gram(X.data_ptr(), n, P, X.stride(0), G.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _lib.stream_ptr(X.device)), "snapshot_gram")
    return G


def snapshot_project(X: torch.Tensor, n: int, P: int, Wt: torch.Tensor) -> torch.Tensor:
    """out [K,P] float64: out[k] = the sequential sum over i of Wt[i,k] * X[i] (Wt float64 [n,K] on X's device, any K >= 1)."""
    if X.dim() != 2 or X.dtype != torch.float32 or not X.is_cuda or X.stride(1) != 1 or X.size(0) < n or X.size(1) < P:
        raise ValueError("snapshot_project: X must be a float32 [rows >= n, columns >= P] device tensor with unit column stride")
    if Wt.dim() != 2 or Wt.dtype != torch.float64 or Wt.device != X.device or Wt.size(0) != n or Wt.size(1) < 1:
        raise ValueError("snapshot_project: Wt must be a float64 [n,K] tensor on X's device")
    lib = _lib.load()
    K = Wt.size(1)
    out = torch.empty([K, P], dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        for k0 in range(0, K, MAX_MODES):                # the entry point takes up to 64 columns: 64 modes and the mean are two calls
            w = Wt[:, k0:k0 + MAX_MODES].contiguous()
            _lib.check(lib.pivlfn_snapshot_project(X.data_ptr(), n, P, X.stride(0), w.data_ptr(), w.size(1), out[k0:].data_ptr(),
                                                   _lib.stream_ptr(X.device)), "snapshot_project")
    return out


class FlowPOD:
    """Collects up to `capacity` flows of H x W (averaged over cell x cell blocks by viz.decimate_flow; cell=1 keeps every vector) as
    rows of a float32 store on the device, and decomposes them."""

    def __init__(self, H: int, W: int, capacity: int, cell: int = 1, device=None):
        check_capacity(capacity)
        if not _args.is_int(cell, 1, 32768):
            raise ValueError(f"FlowPOD: cell={cell!r} must be an integer from 1 to 32768")
        if H < 1 or W < 1:
            raise ValueError(f"FlowPOD: bad flow size {H} x {W}")
        self.H, self.W, self.cell, self.capacity = int(H), int(W), cell, capacity
        self.ch, self.cw = -(-self.H // cell), -(-self.W // cell)
        self.P = 2 * self.ch * self.cw
        self.ld = -(-self.P // 4) * 4
        if self.P >= 1 << 31:
            raise ValueError(f"FlowPOD: {self.P} values per snapshot, must stay below 2^31; use a larger cell")
        self.device = _accum.cuda_device(device)             # a store on the host is refused by update()
        self.store = torch.zeros([capacity, self.ld], dtype=torch.float32, device=self.device)
        self.empty = torch.zeros([], dtype=torch.int64, device=self.device)
        self.n = 0

    @staticmethod
    def store_bytes(H: int, W: int, capacity: int, cell: int = 1) -> int:
        P = 2 * (-(-H // cell)) * (-(-W // cell))
        return capacity * (-(-P // 4) * 4) * 4

    def update(self, flow: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """flow: [B,2,H,W] float32 on this device;  mask: validate_flow's flag bytes [B,H,W] (nonzero = leave the vector out)."""
        from .viz import decimate_flow
        if flow.dim() != 4 or tuple(flow.shape[1:]) != (2, self.H, self.W):
            raise ValueError(f"FlowPOD.update: flows of shape {tuple(flow.shape)}, expected [B,2,{self.H},{self.W}]")
        if flow.device != self.device:
            raise ValueError(f"FlowPOD.update: flows on {flow.device}, the store is on {self.device}")
        B = flow.size(0)
        if self.n + B > self.capacity:
            raise ValueError(f"FlowPOD.update: the store is full ({self.n} of {self.capacity} snapshots, {B} more offered)")
        if B == 0:
            return
        mean, count = decimate_flow(flow, self.cell, mask)
        self.store[self.n:self.n + B, :self.P].copy_(mean.view(B, self.P))
        self.empty += (count == 0).sum()
        self.n += B

    def solve(self, modes: int) -> PODResult:
        n, P = self.n, self.P
        K = check_solve(n, modes, int(self.empty.item()) if n > 0 else 0)
        G = snapshot_gram(self.store, n, P).cpu().numpy()
        lam, V, Wt = solve_gram(G, K)
        out = snapshot_project(self.store, n, P, torch.from_numpy(Wt).to(self.device)).cpu().numpy()
        trace = lam.sum()
        return PODResult(modes=out[:K].reshape(K, 2, self.ch, self.cw), mean=(out[K] / n).reshape(2, self.ch, self.cw),
                         coeff=V * np.sqrt(lam[:K]), energy=lam[:K] / n, fraction=lam[:K] / trace, eigenvalues=lam, gram=G,
                         cell=self.cell, H=self.H, W=self.W)
