"""Oracles of the training frame graph (devo_amd/frame_graph.py), written anew and device-agnostic.

`distance_oracle`, `disps_oracle`, `lists_oracle`: fp64, closed form (no loops over pairs or chunks), in torch.  Pinned against the
reference's own compute_distance_matrix_flow by tests/golden/frame_graph.npz (tools/gen_golden_frame_graph.py) in
tests/test_frame_graph_cpu.py; the oracle of tests/test_gpu_frame_graph.py.

`chunked_distance_matrix`: the reference's composition restated in fp32 torch — chunks of 2048 ordered pairs, both directions per chunk,
one copy to the host per chunk — on whatever device its inputs live: the baseline of tools/bench_frame_graph.py and of one GPU test.

Conventions: poses [N, 7] camera-to-world (tx ty tz qx qy qz qw), disps [N, h, w], intrinsics [N, 4] (fx fy cx cy at the maps'
resolution).  An entry of the matrix is "fragile" when a rounding error can flip a decision: some point of either direction has
|X1_z - 0.2| < 1e-4 (the validity threshold), or the scaled entry lies within 1e-4 * 256 of max_flow (the list threshold)."""
import numpy as np
import torch

MIN_DEPTH = 0.2
MAX_FLOW = 100.0
FRAGILE_Z = 1e-4
FRAGILE_FLOW = 1e-4 * 256


def _rotations(q):
    """[N, 3, 3] of quaternions (x y z w): v -> v + 2 w (u x v) + 2 u x (u x v), the group's action (not normalised, as in the reference)."""
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def directed_sums(poses, disps, intrinsics):
    """fp64: S [N, N] = sum of min(|flow|, 100) over the valid points of i seen from j, V [N, N] (int64) = their number,
    near [N, N] (bool) = some point of i -> j lies within FRAGILE_Z of the validity threshold, peak [N, N] = the largest unclamped flow
    magnitude among the valid points (0 without one)."""
    poses, disps, intrinsics = (torch.as_tensor(t).double() for t in (poses, disps, intrinsics))
    N, h, w = disps.shape
    R, t = _rotations(poses[:, 3:]), poses[:, :3]
    # G_ij = P_j P_i^-1 with P = inverse of camera-to-world: rotation R_j^T R_i, translation R_j^T (t_i - t_j); [i, j, ...]
    Rij = torch.einsum("jkr,akc->ajrc", R, R)
    tij = torch.einsum("jkr,ajk->ajr", R, t[:, None] - t[None, :])
    eye = torch.arange(N, device=disps.device)
    Rij[eye, eye] = torch.eye(3, dtype=torch.float64, device=disps.device)
    tij[eye, eye] = torch.tensor([-0.1, 0.0, 0.0], dtype=torch.float64, device=disps.device)
    ys, xs = torch.meshgrid(torch.arange(h, device=disps.device).double(), torch.arange(w, device=disps.device).double(), indexing="ij")
    fx, fy, cx, cy = (intrinsics[:, k, None, None] for k in range(4))
    X0 = torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(disps)], -1).view(N, h * w, 3)      # [i, p, 3]
    X1 = torch.einsum("ajrc,apc->ajpr", Rij, X0) + tij[:, :, None] * disps.view(N, 1, h * w, 1)           # [i, j, p, 3]
    Z = X1[..., 2]
    Zs = torch.where(Z < 0.5 * MIN_DEPTH, torch.ones_like(Z), Z)
    fj = intrinsics[None, :, None]                                                                       # the target's intrinsics
    u = fj[..., 0] * (X1[..., 0] / Zs) + fj[..., 2] - xs.reshape(-1)
    v = fj[..., 1] * (X1[..., 1] / Zs) + fj[..., 3] - ys.reshape(-1)
    mag = torch.sqrt(u * u + v * v)
    valid = Z > MIN_DEPTH
    S = (mag.clamp(max=MAX_FLOW) * valid).sum(-1)
    V = valid.sum(-1)
    near = ((Z - MIN_DEPTH).abs() < FRAGILE_Z).any(-1)
    peak = (mag * valid).amax(-1)
    return S, V, near, peak


def distance_oracle(poses, disps, intrinsics, scale=1.0, max_flow=256.0):
    """(matrix fp64 [N, N] = scale * (S_ij + S_ji) / (V_ij + V_ji), +inf where fewer than 70 % of the 2 h w points are valid;
    fragile bool [N, N]; tie bool [N, N]: exactly 70 % valid)."""
    S, V, near, _ = directed_sums(poses, disps, intrinsics)
    hw = int(np.prod(disps.shape[1:]))
    Vs = V + V.T
    matrix = scale * (S + S.T) / Vs.clamp(min=1).double()
    matrix[10 * Vs < 14 * hw] = float("inf")
    fragile = near | near.T | ((matrix - max_flow).abs() < FRAGILE_FLOW)
    return matrix, fragile, 10 * Vs == 14 * hw


def disps_oracle(depths):
    """fp64 of base.py:265-268 on [N, h, w]: (1 / depth with every depth below 0.01 replaced by its frame's mean, the replaced mask)."""
    depths = torch.as_tensor(depths)
    low = depths < 0.01                                                                                   # decided on the input's own precision
    d = depths.double()
    mean = d.mean(dim=(1, 2), keepdim=True)
    return 1.0 / torch.where(low, mean.expand_as(d), d), low


def lists_oracle(matrix, max_flow=256.0):
    """CSR (rowptr int64 [N + 1], cols int64, dists) of the entries < max_flow, rows in ascending column order."""
    keep = matrix < max_flow
    rows, cols = keep.nonzero(as_tuple=True)                                                              # row-major: ascending columns per row
    rowptr = torch.zeros(matrix.shape[0] + 1, dtype=torch.int64, device=matrix.device)
    rowptr[1:] = keep.sum(1).cumsum(0)
    return rowptr, cols, matrix[rows, cols]


def rel_dev(a, b):
    """max |a - b| / max(|b|, 1) over the given entries (0 for none)."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / b.abs().clamp(min=1)).max()) if a.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the reference's composition, fp32
def _mul_quat(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def _rotate(q, v):
    u, w = q[..., :3], q[..., 3:]
    c = torch.cross(u, v, dim=-1)
    return v + 2 * w * c + 2 * torch.cross(u, c, dim=-1)


def _inverse(t, q):
    qi = q * q.new_tensor([-1, -1, -1, 1])
    return -_rotate(qi, t), qi


def _induced(t, q, disps, intrinsics, ii, jj, xs, ys):
    """Flow and validity of the pixels of frames ii seen from frames jj: [n, h, w, 2], [n, h, w]; (t, q) world-to-camera."""
    fx, fy, cx, cy = (intrinsics[ii][:, k, None, None] for k in range(4))
    d = disps[ii]
    X0 = torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(d)], -1)
    ti, qi = _inverse(t[ii], q[ii])
    tg, qg = t[jj] + _rotate(q[jj], ti), _mul_quat(q[jj], qi)
    same = ii == jj
    tg[same] = tg.new_tensor([-0.1, 0.0, 0.0])
    qg[same] = qg.new_tensor([0.0, 0.0, 0.0, 1.0])
    X1 = _rotate(qg[:, None, None], X0) + tg[:, None, None] * d[..., None]
    Z = X1[..., 2]
    Zs = torch.where(Z < 0.5 * MIN_DEPTH, torch.ones_like(Z), Z)
    inv = 1.0 / Zs
    fx, fy, cx, cy = (intrinsics[jj][:, k, None, None] for k in range(4))
    coords = torch.stack([fx * (X1[..., 0] * inv) + cx, fy * (X1[..., 1] * inv) + cy], -1)
    return coords - torch.stack([xs, ys], -1), (Z > MIN_DEPTH).float()


def chunked_distance_matrix(poses, disps, intrinsics, chunk=2048):
    """rgbd_utils.compute_distance_matrix_flow as a composition of fp32 torch ops on the inputs' device: all N^2 ordered pairs in chunks,
    both directions per chunk, the chunk's result copied to the host.  -> numpy float32 [N, N]."""
    poses, disps, intrinsics = poses.float(), disps.float(), intrinsics.float()
    dev = disps.device
    N, h, w = disps.shape
    t, q = _inverse(poses[:, :3], poses[:, 3:])
    ys, xs = torch.meshgrid(torch.arange(h, device=dev).float(), torch.arange(w, device=dev).float(), indexing="ij")
    pairs = torch.arange(N * N, device=dev)
    ii, jj = pairs // N, pairs % N
    matrix = np.zeros((N, N), dtype=np.float32)
    for a in range(0, N * N, chunk):
        i, j = ii[a:a + chunk], jj[a:a + chunk]
        flow1, val1 = _induced(t, q, disps, intrinsics, i, j, xs, ys)
        flow2, val2 = _induced(t, q, disps, intrinsics, j, i, xs, ys)
        mag = torch.stack([flow1, flow2], 1).norm(dim=-1).clamp(max=MAX_FLOW).view(len(i), -1)
        val = torch.stack([val1, val2], 1).view(len(i), -1)
        out = (mag * val).mean(-1) / val.mean(-1)
        out[val.mean(-1) < 0.7] = np.inf
        matrix[i.cpu().numpy(), j.cpu().numpy()] = out.cpu().numpy()
    return matrix
