"""dist_chamfer_3D -- differentiable Chamfer3D: the call surface of the reference's external/chamfer3D/dist_chamfer_3D.py.

    dist1, dist2, idx1, idx2 = chamfer_3DFunction.apply(xyz1, xyz2)
    dist1, dist2, idx1, idx2 = chamfer_3DDist()(xyz1, xyz2)

xyz1 [b,n,3], xyz2 [b,m,3] fp32 on one ROCm device.  dist* are the SQUARED nearest-neighbour distances, idx* (int32, not differentiable) the
neighbours' indices, both from chamfer_3D.forward (grid search for large clouds; honours chamfer_3D.SEARCH).  The gradient holds the
indices fixed and flows into both clouds, once: a double backward raises.  Only the gradients autograd asks for are formed.

BACKWARD = "ordered" (default): sc_chamfer3d_backward_ordered (csrc/chamfer_bwd.hip) -- no float atomics, every row summed in a fixed order
(include/shapeclipper_hip.h states it), so the gradient has the same bits run to run, for any batch size, stream or reserved-CU setting.
BACKWARD = "atomic": chamfer_3D.backward on zero-filled buffers, the reference's atomicAdd scatter (sums in arrival order).
There is no CPU fallback: CPU tensors raise.  Kernels go to torch's current stream on the inputs' device.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import chamfer_3D
from shapeclipper_amd import _lib, ops

BACKWARD = "ordered"


def _mode():
    if BACKWARD not in ("ordered", "atomic"):
        raise ValueError("dist_chamfer_3D.BACKWARD must be 'ordered' or 'atomic', got %r" % (BACKWARD,))
    return BACKWARD


def _inputs(xyz1, xyz2):
    if not (xyz1.is_cuda and xyz2.is_cuda):
        raise RuntimeError(_lib.NO_CPU)
    b, n, m = chamfer_3D._dims(xyz1, xyz2)
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
    chamfer_3D._check(xyz1.device, xyz1=(xyz1, torch.float32, (b, n, 3)), xyz2=(xyz2, torch.float32, (b, m, 3)))
    return xyz1, xyz2, b, n, m


class chamfer_3DFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        _mode()                                  # a misspelt setting fails here, not at the first backward
        xyz1, xyz2, b, n, m = _inputs(xyz1, xyz2)
        dev = xyz1.device
        dist1, dist2 = torch.zeros(b, n, device=dev), torch.zeros(b, m, device=dev)      # an empty opposite cloud leaves them untouched
        idx1 = torch.zeros(b, n, dtype=torch.int32, device=dev)
        idx2 = torch.zeros(b, m, dtype=torch.int32, device=dev)
        chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    @once_differentiable
    def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        want1, want2 = ctx.needs_input_grad
        mode = _mode()
        if not (want1 or want2):
            return None, None
        graddist1, graddist2 = graddist1.contiguous(), graddist2.contiguous()
        b, n, m = chamfer_3D._dims(xyz1, xyz2)
        chamfer_3D._check(xyz1.device, graddist1=(graddist1, torch.float32, (b, n)), graddist2=(graddist2, torch.float32, (b, m)))
        with torch.cuda.device(xyz1.device):
            if mode == "ordered":
                g1, g2 = ops.chamfer_backward_ordered(xyz1, xyz2, graddist1, graddist2, idx1, idx2, want1, want2)
            else:
                g1, g2 = torch.zeros_like(xyz1), torch.zeros_like(xyz2)
                chamfer_3D.backward(xyz1, xyz2, g1, g2, graddist1, graddist2, idx1, idx2)
        return (g1 if want1 else None), (g2 if want2 else None)


class chamfer_3DDist(nn.Module):
    def forward(self, input1, input2):
        return chamfer_3DFunction.apply(input1, input2)
