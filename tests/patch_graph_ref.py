"""Plain-torch restatement of the patch-graph bookkeeping of the reference's state machine (devo/devo.py:225-239 append_factors /
remove_factors, :258-265 motionmag, :267-287 and :305-306 keyframe, :289-295 the frame shift), on CPU tensors: test infrastructure,
the yardstick of tests/test_gpu_patch_graph.py.  The reference module itself cannot be imported without a GPU (it builds
`SE3.Identity(1, device="cuda")` at import and pulls in cv2).  The integer side is exact; the magnitudes come from the fp64 oracle
(oracle.pops.flow_mag, pinned to the reference by tests/golden)."""
import torch
from oracle import pops
from oracle.lie import SE3


class RefGraph:
    def __init__(self, M, dim, ix, dtype=torch.float32):
        self.M, self.dim, self.ix = M, dim, ix
        self.ii = torch.zeros(0, dtype=torch.long)
        self.jj = torch.zeros(0, dtype=torch.long)
        self.kk = torch.zeros(0, dtype=torch.long)
        self.net = torch.zeros(1, 0, dim, dtype=dtype)

    def append_factors(self, ii, jj):                                   # devo.py:225-233
        self.jj = torch.cat([self.jj, jj])
        self.kk = torch.cat([self.kk, ii])
        self.ii = torch.cat([self.ii, self.ix[ii]])
        net = torch.zeros(1, len(ii), self.dim, dtype=self.net.dtype)
        self.net = torch.cat([self.net, net], dim=1)

    def remove_factors(self, m):                                        # devo.py:235-239
        self.ii = self.ii[~m]
        self.jj = self.jj[~m]
        self.kk = self.kk[~m]
        self.net = self.net[:, ~m]

    def motionmag(self, poses, patches, intrinsics, i, j, beta=0.5):    # devo.py:258-265, in fp64
        k = (self.ii == i) & (self.jj == j)
        if not bool(k.any()):
            return float("nan")                                         # mean() of an empty tensor (the oracle's SE3 ops refuse empty batches)
        flow = pops.flow_mag(SE3(poses.double()), patches.double(), intrinsics.double(), self.ii[k], self.jj[k], self.kk[k], beta=beta)
        return flow.mean().item()                                       # (NaN for an empty selection, as in the reference)

    def keyframe(self, poses, patches, intrinsics, n, keyframe_index=4, thresh=12.5, removal_window=20):
        """devo.py:267-287, :305-306 on the graph.  Returns (removed, k, m / 2, n after the call)."""
        i = n - keyframe_index - 1
        j = n - keyframe_index + 1
        m = self.motionmag(poses, patches, intrinsics, i, j) + self.motionmag(poses, patches, intrinsics, j, i)
        k = n - keyframe_index
        removed = m / 2 < thresh
        if removed:
            to_remove = (self.ii == k) | (self.jj == k)
            self.remove_factors(to_remove)
            self.kk[self.ii > k] -= self.M
            self.ii[self.ii > k] -= 1
            self.jj[self.jj > k] -= 1
            n -= 1
        to_remove = self.ix[self.kk] < n - removal_window
        self.remove_factors(to_remove)
        return removed, k, m / 2, n


def shift_frames(tensors, k, n):                                        # devo.py:289-295
    for i in range(k, n - 1):
        for t in tensors:
            t[i] = t[i + 1]
