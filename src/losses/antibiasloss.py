"""AntibiasLoss -- drop-in for reference src/losses/antibiasloss.py (:4-14): L1 between the 2^n x 2^n average-pooled images, value and
gradient from the HIP objective kernel (diner_objective_f32 with the MSE term off)."""
import torch


class AntibiasLoss(torch.nn.Module):
    def __init__(self, n_downsampling, metric=torch.nn.L1Loss()):
        super().__init__()
        if not (isinstance(metric, torch.nn.L1Loss) and metric.reduction == "mean"):
            raise NotImplementedError("diner_amd: AntibiasLoss runs torch.nn.L1Loss() (mean), the reference's default, on the device")
        self.n_downsampling = int(n_downsampling)
        self.metric = metric

    def forward(self, x, y):
        """x, y (N,3,s,s) on a HIP device, s a multiple of 2^n_downsampling -> 0-dim loss, differentiable with respect to x."""
        from diner_amd import objective
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or y.shape != x.shape:
            raise ValueError(f"diner_amd: AntibiasLoss expects two (N,3,s,s) tensors, got {tuple(x.shape)}, {tuple(y.shape)}")
        N, _, s, _ = x.shape
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(N, s * s, 3)
        return objective.photometric(rows(x), rows(y.detach()), s, self.n_downsampling, w_antibias=1.0, w_mse=0.0).total
