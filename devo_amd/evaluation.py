"""Trajectory evaluation on the GPU over csrc/traj_eval.hip: what the reference's utils/eval_utils.py (`ate`, `ate_real`, `log_results`,
`compute_median_results`) obtains from evo — the association of an estimated and a ground-truth trajectory by their stamps, the Umeyama
alignment (Umeyama 1991) and the absolute trajectory error with its statistics — as ONE launch for a whole batch of pairs, one workgroup
per pair, all arithmetic in fp64, bit-reproducible and independent of the batch.

A pair is an estimate (poses [Ne, 7] as t, q_xyzw, camera-to-world; stamps [Ne]) and a ground truth ([Ng, 7], [Ng]).  Poses are fp32 or
fp64, stamps int64 (microseconds) or fp64; stamps are compared after conversion to fp64, which is exact below 2^53 (numpy stamps beyond
are refused here, device stamps beyond flag their pair).  `Trajectory.complete`'s output goes in as it is.

  * association "nearest": the shorter trajectory (the ground truth at equal length) is the short one; short pose i takes the long pose
    whose stamp is nearest (the lowest index on equal distance, the leftmost of equal stamps) and is kept when the distance is <= max_diff.
    "interpolate": every estimated stamp inside the ground truth's range gets the ground truth interpolated there (linear translation,
    shorter-arc slerp); `max_diff` is not used.  The long stamps must be non-decreasing.  The reference's cubic translation spline
    (pose_utils.interpolate_traj_at_tss) is not built; the reference has it commented out.
  * alignment "none" | "se3" | "sim3" of the estimate onto the ground truth over the matched positions; R is always a proper rotation
    (the reflection correction), a planar trajectory is valid, fewer than three matches or sigma_2 <= 1e-10 sigma_1 is degenerate.
  * quaternions are read as xyzw.  The reference hands its xyzw quaternions to an interface that takes wxyz (its own TODO); the
    translation ATE — the figure it reports — does not depend on them, the rotation columns here are those of the poses as documented.

The columns of `Result.stats` (fp64 [B, 16]), each also an attribute of the result: see COLUMNS; e_i = |y_i - (c R x_i + t)|.  `transform`
is fp64 [B, 8] = (c, t, q_xyzw of R), `status` int32 [B] of FLAGS bits.  A flagged pair has NaN in every column but `n` and in its
transform; with check=True (one read-back of `status`) it raises instead, naming the pair.

No CPU fallback: CPU tensors raise; numpy arrays are uploaded.  One launch per call, on the current stream; the only host synchronisation
is the status read-back of check=True.  Lists of tensors are packed on the device (one concatenation each); the offsets are built on the
host and uploaded (one small copy).

`relative_errors` (csrc/traj_rel.hip) is the relative pose error over sub-trajectories of given lengths in frames, seconds, metres, radians
or degrees: what the reference's scripts/evaluate_rpe.py computes for a fixed delta and what its log_results calls the "rel stats".  See the
function; REL_COLUMNS are the columns of `RelativeResult.stats` (fp64 [B, D, 16]).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import backends

COLUMNS = ("n", "rmse", "mean", "median", "std", "min", "max", "sse", "rot_rmse_deg", "rot_mean_deg", "path_length", "mpe", "scale", "rpe_trans_rmse",
           "rpe_rot_rmse_deg", "rpe_terms")                         # DEVO_TRAJ_EVAL_COLS
MAX_MATCHES = 1 << 17                                              # DEVO_TRAJ_EVAL_MAX_MATCHES: short poses per pair
ALIGN = {"none": 0, "se3": 1, "sim3": 2}                           # DEVO_TRAJ_ALIGN_*
ASSOCIATION = {"nearest": 0, "interpolate": 1}                     # DEVO_TRAJ_ASSOC_*
FLAGS = {1: "no stamp of the short trajectory has a partner within max_diff", 2: "fewer than three matches", 4: "degenerate: the matched positions are collinear or coincide",
         8: "the long trajectory's stamps are not non-decreasing", 16: f"more than {MAX_MATCHES} poses in the short trajectory",
         32: "a stamp is not finite or its magnitude is 2^53 or more", 64: "offsets outside the packed tensors"}   # DEVO_TRAJ_*
_STAMP_LIMIT = float(1 << 53)


class Result:
    """stats fp64 [B, 16] (COLUMNS; every column is an attribute: result.rmse is stats[:, 1]), transform fp64 [B, 8], status int32 [B];
    errors fp64 / matched int32 [total_est] or None, packed like the estimate: `errors_of(b)`, `matched_of(b)` give pair b's rows, one per
    SHORT pose (NaN / -1 where unmatched).  short_is_est[b] says which trajectory of pair b is the short one."""

    def __init__(self, stats, transform, status, errors, matched, est_offsets, gt_offsets, short_is_est):
        self.stats, self.transform, self.status, self.errors, self.matched = stats, transform, status, errors, matched
        self.est_offsets, self.gt_offsets, self.short_is_est = est_offsets, gt_offsets, short_is_est

    def __getattr__(self, name):
        if name in COLUMNS:
            return self.stats[:, COLUMNS.index(name)]
        raise AttributeError(name)

    def __len__(self):
        return self.stats.shape[0]

    def _rows(self, t, b):
        if t is None:
            raise ValueError("evaluate: ask for it (return_errors=True / return_matches=True)")
        o = self.est_offsets[b]
        n = (self.est_offsets if self.short_is_est[b] else self.gt_offsets)
        return t[o:o + n[b + 1] - n[b]]

    def errors_of(self, b=0):
        return self._rows(self.errors, b)

    def matched_of(self, b=0):
        return self._rows(self.matched, b)

    def sim3(self):
        """The alignments as a `lietorch.Sim3` of shape [B] (fp64, data = (t, q_xyzw, c)): `S.act(x)` is c R x + t, and it composes, inverts
        and differentiates like any group element.  A flagged pair stays NaN."""
        from .lietorch import Sim3
        return Sim3(torch.cat([self.transform[:, 1:8], self.transform[:, 0:1]], -1))


def _device(*groups):
    for g in groups:
        for t in (g if isinstance(g, (list, tuple)) else (g,)):
            if torch.is_tensor(t) and t.is_cuda:
                return t.device
    return None                                                    # (numpy only: the current device, resolved by the upload)


def _upload(t, dev, what):
    """numpy -> device; tensors must be on the GPU already"""
    if isinstance(t, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(t)).to(dev if dev is not None else "cuda")
    if not torch.is_tensor(t):
        raise TypeError(f"evaluate: {what} must be tensors or numpy arrays, not {type(t).__name__}")
    L.require_gpu(t)
    return t


def _pack(x, dev, what):
    """one tensor or a list of them -> (packed tensor, lengths or None)"""
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError("evaluate: an empty list of trajectories")
        parts = [_upload(t, dev, what) for t in x]
        dt = torch.float64 if any(p.dtype == torch.float64 for p in parts) else parts[0].dtype
        parts = [p.to(dt) for p in parts]
        return (torch.cat(parts, 0) if len(parts) > 1 else parts[0]), [int(p.shape[0]) for p in parts]
    return _upload(x, dev, what), None


def _offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def _host_offsets(o, total, what):
    if torch.is_tensor(o):
        o = o.tolist()
    o = [int(v) for v in (o.tolist() if isinstance(o, np.ndarray) else o)]
    if len(o) < 2 or o[0] != 0 or o[-1] != total or any(b < a for a, b in zip(o, o[1:])):
        raise ValueError(f"evaluate: {what} offsets must rise from 0 to the number of packed poses ({total})")
    return o


def _inputs(est, est_stamps, gt, gt_stamps, offsets):
    """what `evaluate` and `relative_errors` accept -> packed device tensors of matching dtypes and the host offsets:
    (est, est_stamps, gt, gt_stamps, est_offsets, gt_offsets)"""
    for stamps in (est_stamps, gt_stamps):                         # what the host can see of the stamps, before anything is uploaded
        for t in (stamps if isinstance(stamps, (list, tuple)) else (stamps,)):
            if isinstance(t, np.ndarray) and t.size and not float(np.abs(t.astype(np.float64)).max()) < _STAMP_LIMIT:
                raise ValueError("evaluate: a stamp is not finite or its magnitude is 2^53 or more (stamps are compared in fp64)")
    dev = _device(est, est_stamps, gt, gt_stamps)
    est, ne = _pack(est, dev, "poses")
    est_stamps, ne_t = _pack(est_stamps, dev, "stamps")
    gt, ng = _pack(gt, dev, "poses")
    gt_stamps, ng_t = _pack(gt_stamps, dev, "stamps")
    dev = est.device
    if ne != ne_t or ng != ng_t or (ne is None) != (ng is None) or (ne is not None and len(ne) != len(ng)):
        raise ValueError("evaluate: poses and stamps must come as matching lists, one entry per pair")
    for t in (est, gt):
        if t.dim() != 2 or t.shape[1] != 7 or t.dtype not in (torch.float32, torch.float64):
            raise ValueError("evaluate: poses must be float32 or float64 [N, 7] (t, q_xyzw)")
    if est.dtype != gt.dtype:
        est, gt = est.double(), gt.double()
    for t, p in ((est_stamps, est), (gt_stamps, gt)):
        if t.dim() != 1 or t.shape[0] != p.shape[0]:
            raise ValueError("evaluate: one stamp per pose expected")
        if t.device != dev or p.device != dev:
            raise ValueError("evaluate: all tensors must live on one GPU")

    def stamp_type(t):
        if t.dtype in (torch.int64, torch.float64):
            return t
        if t.dtype in (torch.int32, torch.int16, torch.uint8, torch.int8):
            return t.long()
        if t.dtype in (torch.float32, torch.float16, torch.bfloat16):
            return t.double()                                        # exact
        raise ValueError(f"evaluate: stamps of dtype {t.dtype}")
    est_stamps, gt_stamps = stamp_type(est_stamps), stamp_type(gt_stamps)
    if est_stamps.dtype != gt_stamps.dtype:
        est_stamps, gt_stamps = est_stamps.double(), gt_stamps.double()      # (an int64 of 2^53 or more stays at or above 2^53: the kernel flags it)
    if ne is not None:
        if offsets is not None:
            raise ValueError("evaluate: offsets go with packed tensors, not with lists")
        eo, go = _offsets(ne), _offsets(ng)
    elif offsets is not None:
        eo, go = _host_offsets(offsets[0], est.shape[0], "the estimate's"), _host_offsets(offsets[1], gt.shape[0], "the ground truth's")
        if len(eo) != len(go):
            raise ValueError("evaluate: the two offset vectors must have the same length B + 1")
    else:
        eo, go = [0, est.shape[0]], [0, gt.shape[0]]
    return est.contiguous(), est_stamps.contiguous(), gt.contiguous(), gt_stamps.contiguous(), eo, go


def evaluate(est, est_stamps, gt, gt_stamps, *, max_diff, align="sim3", association="nearest", rpe_delta=0, offsets=None, return_errors=False, return_matches=False,
             check=True):
    """One pair (est [Ne, 7], est_stamps [Ne], gt [Ng, 7], gt_stamps [Ng]), lists of those (one entry per pair), or packed tensors with
    offsets=(est_offsets, gt_offsets), two host sequences of B + 1 row offsets.  max_diff is in the stamps' unit.  -> Result."""
    if align not in ALIGN:
        raise ValueError(f"evaluate: align {align!r} (have: none, se3, sim3)")
    if association not in ASSOCIATION:
        raise ValueError(f"evaluate: association {association!r} (have: nearest, interpolate)")
    max_diff, rpe_delta = float(max_diff), int(rpe_delta)
    if association == "nearest" and not max_diff >= 0.0:
        raise ValueError("evaluate: max_diff must be >= 0")
    if rpe_delta < 0:
        raise ValueError("evaluate: rpe_delta must be >= 0")
    est, est_stamps, gt, gt_stamps, eo, go = _inputs(est, est_stamps, gt, gt_stamps, offsets)
    dev = est.device
    B = len(eo) - 1
    interp = association == "interpolate"
    short_is_est = [interp or (eo[b + 1] - eo[b]) < (go[b + 1] - go[b]) for b in range(B)]
    total_est = est.shape[0]
    with torch.cuda.device(dev):
        off = torch.tensor([eo, go], dtype=torch.int64).to(dev, non_blocking=True)
        nat = backends.native()
        if nat is not None:
            stats, transform, status, errors, matched = nat.evaluation.traj_eval(est, est_stamps, off[0], gt, gt_stamps, off[1], ASSOCIATION[association], ALIGN[align],
                                                                                 max_diff, rpe_delta, bool(return_errors), bool(return_matches))
        else:
            stats = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=dev)
            transform = torch.empty((B, 8), dtype=torch.float64, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            errors = torch.empty(total_est if return_errors else 0, dtype=torch.float64, device=dev)
            matched = torch.empty(total_est if return_matches else 0, dtype=torch.int32, device=dev)
            bytes_ = int(L.lib().devo_traj_eval_workspace_bytes(total_est, ASSOCIATION[association]))
            ws = torch.empty(bytes_, dtype=torch.uint8, device=dev)
            rc = L.lib().devo_traj_eval(L.ptr(est), L.ptr(est_stamps), L.ptr(off[0]), total_est, L.ptr(gt), L.ptr(gt_stamps), L.ptr(off[1]), gt.shape[0], B,
                                        L.dtype_code(est), int(est_stamps.dtype == torch.float64), ASSOCIATION[association], ALIGN[align], max_diff, rpe_delta,
                                        L.ptr(stats), L.ptr(transform), L.ptr(status), L.ptr(errors) if return_errors else None,
                                        L.ptr(matched) if return_matches else None, L.ptr(ws), bytes_, L.stream())
            L.check(rc, "evaluate")
        if check and not torch.cuda.is_current_stream_capturing():
            for b, s in enumerate(status.tolist()):                                      # the one read-back
                if s:
                    why = "; ".join(text for bit, text in FLAGS.items() if s & bit)
                    raise RuntimeError(f"evaluate: pair {b} ({eo[b + 1] - eo[b]} estimated, {go[b + 1] - go[b]} ground-truth poses): {why}")
    return Result(stats, transform, status, errors if return_errors else None, matched if return_matches else None, eo, go, short_is_est)


def ate(traj_ref, traj_est, timestamps=None):
    """eval_utils.ate (the reference's argument order): the RMSE of the translation error after a Sim(3) alignment, in the poses' unit,
    of two trajectories of equal length paired pose by pose (the stamps are not looked at, as in the reference, where both get the same)."""
    n = len(traj_ref)
    if len(traj_est) != n:
        raise ValueError(f"ate: {n} reference poses against {len(traj_est)} estimated ones (ate_real associates by stamps)")
    dev = _device(traj_ref, traj_est)
    idx = torch.arange(n, dtype=torch.int64, device=dev) if dev is not None else np.arange(n, dtype=np.int64)
    return float(evaluate(traj_est, idx, traj_ref, idx, max_diff=0).rmse[0])


def ate_real(traj_ref, tss_ref_us, traj_est, tstamps):
    """eval_utils.ate_real: stamps in microseconds, nearest association within one second, Sim(3) alignment -> (ATE in cm for poses in metres,
    the matched reference poses, the matched estimated poses), the last two as device tensors [n, 7] in matching order."""
    dev = _device(traj_ref, tss_ref_us, traj_est, tstamps)
    ref, est = _upload(traj_ref, dev, "poses"), _upload(traj_est, dev, "poses")
    if ref.shape == est.shape:
        t_ref, t_est = _upload(tss_ref_us, dev, "stamps"), _upload(tstamps, dev, "stamps")
        if not bool((t_ref == t_est).all()):
            raise ValueError("ate_real: trajectories of equal length must share their stamps")
        return ate(ref, est) * 100.0, ref, est
    r = evaluate(est, tstamps, ref, tss_ref_us, max_diff=1e6, return_matches=True)
    m = r.matched_of(0)
    short = torch.nonzero(m >= 0).squeeze(1)
    long = m[short].long()
    i_est, i_ref = (short, long) if r.short_is_est[0] else (long, short)
    return float(r.rmse[0]) * 100.0, ref[i_ref], est[i_est]


def summary(results_by_scene, dataset_name=None):
    """eval_utils.compute_median_results on {scene: [ATE in cm per trial]} -> {scene (or dataset/scene): the median, "AUC": mean(max(1 - x, 0))
    over all results, "AVG": the mean of the medians in m}."""
    if not results_by_scene:
        raise ValueError("summary: no results")
    out, medians, everything = {}, [], []
    for scene, values in results_by_scene.items():
        v = torch.as_tensor([float(x) for x in values], dtype=torch.float64)
        if v.numel() == 0:
            raise ValueError(f"summary: scene {scene!r} has no result")
        s = v.sort().values
        med = float(0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2]))                         # numpy's median
        out[f"{dataset_name}/{scene}" if dataset_name else scene] = med
        medians.append(med)
        everything.append(v)
    out["AUC"] = float(torch.clamp(1.0 - torch.cat(everything), min=0.0).mean())
    out["AVG"] = sum(medians) / len(medians) / 100.0
    return out


# ---------------------------------------------------------------------------------------------------------------- relative pose error
REL_COLUMNS = ("n", "trans_rmse", "trans_mean", "trans_median", "trans_std", "trans_min", "trans_max", "rot_rmse_deg", "rot_mean_deg", "rot_median_deg",
               "rot_std_deg", "rot_min_deg", "rot_max_deg", "delta", "span_mean", "scale")      # DEVO_TRAJ_REL_COLS
MAX_DELTAS = 16                                                    # DEVO_TRAJ_REL_MAX_DELTAS
UNITS = {"f": 0, "s": 1, "m": 2, "rad": 3, "deg": 4}               # DEVO_TRAJ_REL_UNIT_*
ALONG = {"gt": 0, "est": 1}                                        # DEVO_TRAJ_REL_ALONG_*
END = {"reach": 0, "closest": 1}                                   # DEVO_TRAJ_REL_END_*
NO_PAIR = 128                                                      # DEVO_TRAJ_REL_NO_PAIR
REL_FLAGS = dict(FLAGS)
REL_FLAGS.update({2: "too few matches (three for scale=\"sim3\", two for a given scale)", 8: "the long trajectory's stamps, or the estimate's matched stamps, are not non-decreasing",
                  NO_PAIR: "no sub-trajectory of this length (no pair of poses)"})


class RelativeResult:
    """stats fp64 [B, D, 16] (REL_COLUMNS; every column is an attribute: result.trans_rmse is stats[:, :, 1]), status int32 [B, D];
    errors fp64 [D, total_est, 2] (|t_E|, the angle of R_E in degrees) / ends int32 [D, total_est] or None, packed like the estimate:
    `errors_of(b, d)`, `ends_of(b, d)` give pair b's rows for delta d, row i for the sub-trajectory that starts at match i (NaN / -1
    where there is none, and behind the number of matches); an end is a match number as well."""

    def __init__(self, stats, status, errors, ends, est_offsets, unit):
        self.stats, self.status, self.errors, self.ends, self.est_offsets, self.unit = stats, status, errors, ends, est_offsets, unit

    def __getattr__(self, name):
        if name in REL_COLUMNS:
            return self.stats[:, :, REL_COLUMNS.index(name)]
        raise AttributeError(name)

    def __len__(self):
        return self.stats.shape[0]

    def _rows(self, t, b, d):
        if t is None:
            raise ValueError("relative_errors: ask for it (return_errors=True)")
        return t[d, self.est_offsets[b]:self.est_offsets[b + 1]]

    def errors_of(self, b=0, d=0):
        return self._rows(self.errors, b, d)

    def ends_of(self, b=0, d=0):
        return self._rows(self.ends, b, d)

    def percent(self):
        """RPG's relative figures for unit "m" -> (100 trans_mean / delta in percent, rot_mean_deg / delta in degrees per metre), each [B, D]"""
        if self.unit != "m":
            raise ValueError(f"percent: the deltas are in {self.unit!r}, not in metres")
        return 100.0 * self.trans_mean / self.delta, self.rot_mean_deg / self.delta


def relative_errors(est, est_stamps, gt, gt_stamps, *, deltas, unit="m", relative=False, along="gt", end="reach", scale="sim3", max_diff, association="nearest",
                    offsets=None, return_errors=False, check=True):
    """The relative pose error over sub-trajectories of the lengths `deltas` (1 .. 16 positive numbers in `unit`: "f" frames, i.e. matches,
    "s" the stamps' unit, "m", "rad", "deg"; with relative=True fractions of the whole index range, resolved on the device).  Inputs as for
    `evaluate`; the stages for a pair:
      1. association, exactly `evaluate`'s -> n matches (x_k, y_k, s_k) in short order, s_k the estimate's stamp;
      2. the scale c of the estimate's relative translations: "sim3" (the Umeyama scale, `evaluate(align="sim3").scale`), a float for all
         pairs, or a device tensor [B]; a given scale needs two matches and no alignment;
      3. the index u_k: k, s_k, or the cumulative path length / rotation angle along the matched ground truth (along="gt", the RPG
         convention) or the estimate (along="est", scripts/evaluate_rpe.py; its lengths times c);
      4. the end j of the sub-trajectory that starts at i: end="reach", the first j > i with u_j - u_i >= delta; end="closest", the j
         nearest to u_i + delta (the lowest on a tie), dropped when j = n - 1 (evaluate_rpe.py:263-266);
      5. E = (c . (X_i^-1 X_j))^-1 (Y_i^-1 Y_j): |t_E| and the angle of R_E in degrees;
      6. the statistics per (pair, delta) -> RelativeResult.
    Three launches on the current stream (csrc/traj_rel.hip); the only host synchronisation is the status read-back of check=True, which
    raises for a flagged pair or a (pair, delta) without a pair of poses, naming both."""
    who = "relative_errors"
    if association not in ASSOCIATION:
        raise ValueError(f"{who}: association {association!r} (have: nearest, interpolate)")
    if unit not in UNITS:
        raise ValueError(f"{who}: unit {unit!r} (have: f, s, m, rad, deg)")
    if along not in ALONG:
        raise ValueError(f"{who}: along {along!r} (have: gt, est)")
    if end not in END:
        raise ValueError(f"{who}: end {end!r} (have: reach, closest)")
    max_diff = float(max_diff)
    if association == "nearest" and not max_diff >= 0.0:
        raise ValueError(f"{who}: max_diff must be >= 0")
    deltas = [float(v) for v in (deltas if isinstance(deltas, (list, tuple, np.ndarray)) else (deltas,))]
    D = len(deltas)
    if not 1 <= D <= MAX_DELTAS:
        raise ValueError(f"{who}: 1 .. {MAX_DELTAS} deltas expected ({D})")
    if not all(0.0 < v < float("inf") for v in deltas):
        raise ValueError(f"{who}: deltas must be positive and finite ({deltas})")
    B = len(est) if isinstance(est, (list, tuple)) else len(offsets[0]) - 1 if offsets is not None else 1      # (checked again by the packing)
    scales, scale_value = None, 1.0
    if isinstance(scale, str):
        if scale != "sim3":
            raise ValueError(f"{who}: scale {scale!r} (have: \"sim3\", a float, a device tensor [B])")
        mode = 0
    elif torch.is_tensor(scale):
        if scale.dim() != 1 or scale.shape[0] != B or not scale.is_floating_point():
            raise ValueError(f"{who}: a scale tensor must hold one floating-point number per pair ([{B}]), not {tuple(scale.shape)} of {scale.dtype}")
        L.require_gpu(scale)
        scales, mode = scale.double().contiguous(), 2
    else:
        scale_value, mode = float(scale), 1
        if not 0.0 < scale_value < float("inf"):
            raise ValueError(f"{who}: the scale must be positive and finite ({scale_value})")
    est, est_stamps, gt, gt_stamps, eo, go = _inputs(est, est_stamps, gt, gt_stamps, offsets)
    dev = est.device
    if len(eo) - 1 != B or (scales is not None and scales.device != dev):
        raise ValueError(f"{who}: one scale per pair on the poses' GPU expected")
    total_est = est.shape[0]
    with torch.cuda.device(dev):
        off = torch.tensor([eo, go], dtype=torch.int64).to(dev, non_blocking=True)
        nat = backends.native()
        if nat is not None:
            stats, status, errors, ends = nat.evaluation.traj_rel_eval(est, est_stamps, off[0], gt, gt_stamps, off[1], ASSOCIATION[association], max_diff, deltas,
                                                                       UNITS[unit], bool(relative), ALONG[along], END[end], mode, scale_value, scales, bool(return_errors))
        else:
            stats = torch.empty((B, D, len(REL_COLUMNS)), dtype=torch.float64, device=dev)
            status = torch.empty((B, D), dtype=torch.int32, device=dev)
            errors = torch.empty((D, total_est, 2) if return_errors else 0, dtype=torch.float64, device=dev)
            ends = torch.empty((D, total_est) if return_errors else 0, dtype=torch.int32, device=dev)
            bytes_ = int(L.lib().devo_traj_rel_workspace_bytes(total_est, ASSOCIATION[association], B, D))
            ws = torch.empty(bytes_, dtype=torch.uint8, device=dev)
            rc = L.lib().devo_traj_rel_eval(L.ptr(est), L.ptr(est_stamps), L.ptr(off[0]), total_est, L.ptr(gt), L.ptr(gt_stamps), L.ptr(off[1]), gt.shape[0], B,
                                            L.dtype_code(est), int(est_stamps.dtype == torch.float64), ASSOCIATION[association], max_diff, (ctypes.c_double * D)(*deltas), D,
                                            UNITS[unit], int(bool(relative)), ALONG[along], END[end], mode, scale_value, L.ptr(scales), L.ptr(stats), L.ptr(status),
                                            L.ptr(errors) if return_errors else None, L.ptr(ends) if return_errors else None, L.ptr(ws), bytes_, L.stream())
            L.check(rc, who)
        if check and not torch.cuda.is_current_stream_capturing():
            for b, row in enumerate(status.tolist()):                                    # the one read-back
                for d, s in enumerate(row):
                    if s:
                        why = "; ".join(text for bit, text in REL_FLAGS.items() if s & bit)
                        raise RuntimeError(f"{who}: pair {b} ({eo[b + 1] - eo[b]} estimated, {go[b + 1] - go[b]} ground-truth poses), delta {d} ({deltas[d]:g} {unit}"
                                           f"{', relative' if relative else ''}): {why}")
    return RelativeResult(stats, status, errors if return_errors else None, ends if return_errors else None, eo, unit)
