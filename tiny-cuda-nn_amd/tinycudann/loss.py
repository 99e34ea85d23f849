"""The library's losses in a torch training loop: `tinycudann.Loss(otype)` (L2, RelativeL2, RelativeL2Luminance, L1, RelativeL1, Mape,
Smape, CrossEntropy, Variance; reference losses/*.h) evaluates value and gradient in ONE native kernel launch (tcnn_loss_evaluate /
tcnn_loss_evaluate_precision) behind a torch.autograd.Function.

`loss(prediction, target, data_pdf=None)`: prediction [n, dims] float32 (the fp32 kernel) or the library's 16-bit type (the 16-bit kernel),
target / data_pdf [n, dims] float32 -> the scalar mean loss (the sum of the per-element values, normalised by n * dims: what
Trainer::loss reports).  Backward gives the kernel's gradient (loss_scale = 1) times the incoming scalar; target and data_pdf carry none.
The kernels want the prediction's width padded to a multiple of 8: narrower predictions are padded here, the added columns carry no
loss; any n is taken as it is (the kernels need no batch granularity, and the mean is over the caller's n * dims)."""
import torch

from . import _C


def _prepare(otype, prediction, target, data_pdf):
    if prediction.dim() != 2:
        raise RuntimeError("tinycudann.Loss: prediction must be [n, dims]")
    if not prediction.is_cuda:
        raise RuntimeError("tinycudann.Loss: prediction must live on the GPU")
    if prediction.dtype != torch.float32 and prediction.dtype != _C.TORCH_DTYPE[_C.preferred_precision()]:
        raise RuntimeError(f"tinycudann.Loss: prediction must be float32 or {_C.TORCH_DTYPE[_C.preferred_precision()]}")
    n, dims = prediction.shape
    for name, t in (("target", target), ("data_pdf", data_pdf)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, dims):
            raise RuntimeError(f"tinycudann.Loss: {name} must be a float32 GPU tensor of the prediction's shape")
    target = target.detach().contiguous()
    data_pdf = None if data_pdf is None else data_pdf.detach().contiguous()
    padded = (dims + 7) // 8 * 8
    p = prediction.detach()
    p = torch.nn.functional.pad(p, (0, padded - dims)) if padded != dims else p.contiguous()
    return p, target, data_pdf, dims


def _evaluate(otype, prediction, target, data_pdf):
    """-> (values [n, dims] float32, gradients [n, dims] in the prediction's dtype), loss_scale = 1"""
    p, target, data_pdf, dims = _prepare(otype, prediction, target, data_pdf)
    with _C._DeviceGuard(p.device):
        values, gradients = _C.loss_evaluate(otype, p, target, loss_scale=1.0, data_pdf=data_pdf)
    return values[:, :dims], gradients[:, :dims]


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, otype, prediction, target, data_pdf):
        values, gradients = _evaluate(otype, prediction, target, data_pdf)
        ctx.save_for_backward(gradients)
        return values.sum()

    @staticmethod
    def backward(ctx, grad_output):
        (gradients,) = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[1]:
            grad = (gradients * grad_output.to(gradients.dtype)).contiguous()
        return None, grad, None, None


class Loss(torch.nn.Module):
    def __init__(self, otype):
        super().__init__()
        self.otype = str(otype)

    def forward(self, prediction, target, data_pdf=None):
        return _LossFunction.apply(self.otype, prediction, target, data_pdf)

    @torch.no_grad()
    def values(self, prediction, target, data_pdf=None):
        """the per-element loss values [n, dims] (float32); their sum is forward()'s result"""
        return _evaluate(self.otype, prediction, target, data_pdf)[0].contiguous()

    def extra_repr(self):
        return f"otype={self.otype}"
