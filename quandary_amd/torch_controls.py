"""Sampled controls as a differentiable torch function: the objective of Optim.evalGradF_sampled as a 0-d tensor whose backward pass
hands d objective / d sample to whatever produced the samples (a filter chain, a pulse-generating model)."""
import torch


class SampledObjective(torch.autograd.Function):
    """objective = SampledObjective.apply(samples, optim, mode): samples is a [nsamp, nosc, 2] float64 tensor of (p, q) in rad/ns on any
    device (copied to the host), optim a capi.Optim, mode 'rows' | 'hold' | 'linear'.  Both sweeps run in forward(); backward() scales
    the saved gradient."""

    @staticmethod
    def forward(ctx, samples, optim, mode="rows"):
        if samples.dtype != torch.float64 or samples.dim() != 3:
            raise TypeError("SampledObjective: samples must be a [nsamp, nosc, 2] float64 tensor")
        val, grad = optim.evalGradF_sampled(samples.detach().cpu().contiguous().numpy(), mode)
        ctx.save_for_backward(torch.from_numpy(grad).to(samples.device))
        return torch.tensor(val["objective"], dtype=torch.float64, device=samples.device)

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output, None, None
