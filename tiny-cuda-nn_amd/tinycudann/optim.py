"""The library's optimizers in a torch training loop: `tinycudann.optim.Optimizer(modules, config)` is a `torch.optim.Optimizer` that steps
the fp32 `params` of tinycudann modules with the native optimizer chains (Adam, SGD, Novograd under any order of Ema, ExponentialDecay,
Lookahead, Average, Batched; `config` is the "optimizer" block of the reference's JSON) -- the fp32 instantiation of the kernels the
trainer steps with (`native.Optimizer(..., precision=Precision.Fp32)`, tcnn_create_optimizer_precision).

    model = tcnn.NetworkWithInputEncoding(...)
    opt = tcnn.optim.Optimizer(model, {"otype": "Ema", "decay": 0.99, "nested": {"otype": "Adam", "learning_rate": 1e-2}})
    loss = tcnn.Loss("RelativeL2")(model(x), target); loss.backward(); opt.step(); opt.zero_grad()
    model_for_inference_params = opt.inference_params(model)   # Ema's average

Each module gets one native optimizer sized by `module.params.numel()`, with the module's network weight matrices (`network_layers()`) as
Adam's matrix parameters / Novograd's layers; the rest of the vector (an encoding's parameters) are non-matrix parameters: per-parameter
step counters, `skip_zero_grad_non_matrix_params`, `non_matrix_learning_rate_factor` apply to them as in the trainer."""
import copy

import torch

from . import _C, native


def _check_tensor(what, t):
    if not t.is_cuda:
        raise RuntimeError(f"tinycudann.optim: {what} must live on the GPU")
    if t.dtype != torch.float32:
        raise RuntimeError(f"tinycudann.optim: {what} must be float32")
    if not t.is_contiguous():
        raise RuntimeError(f"tinycudann.optim: {what} must be contiguous")


class Optimizer(torch.optim.Optimizer):
    def __init__(self, modules, config):
        modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        if not modules:
            raise ValueError("tinycudann.optim.Optimizer: no modules")
        for m in modules:
            if not hasattr(m, "native_tcnn_module") or not hasattr(m, "params"):
                raise TypeError("tinycudann.optim.Optimizer steps tinycudann modules (Encoding, Network, NetworkWithInputEncoding)")
            _check_tensor("a module's params", m.params.data)
        self._modules = modules
        self._config = copy.deepcopy(config)
        self._native = []
        for m in modules:
            with torch.cuda.device(m.params.device):
                self._native.append(native.Optimizer(config, m.params.numel(), layer_sizes=m.native_tcnn_module.network_layers(), precision=_C.Precision.Fp32))
        super().__init__([{"params": [m.params]} for m in modules], {})

    def _index(self, module):
        for i, m in enumerate(self._modules):
            if m is module:
                return i
        raise KeyError("tinycudann.optim.Optimizer: not one of this optimizer's modules")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for m, opt in zip(self._modules, self._native):
            p = m.params
            if p.grad is None:  # (its step count does not advance)
                continue
            _check_tensor("a module's params", p.data)
            _check_tensor("a module's params.grad", p.grad)
            with _C._DeviceGuard(p.device):
                opt.step(p.data, None, p.grad, 1.0)  # the binding has divided its loss scale out of the gradient already
        return loss

    def native_optimizer(self, module):
        return self._native[self._index(module)]

    def step_count(self, module):
        return self._native[self._index(module)].step_count

    def hyperparams(self):
        """Optimizer::hyperparams() (the same for every module)"""
        return self._native[0].hyperparams()

    def update_hyperparams(self, config):
        for opt in self._native:
            opt.update_hyperparams(config)

    def inference_params(self, module):
        """The outermost wrapper's custom weights (Ema's average, Lookahead's slow weights, Average's mean) as a float32 view of the native
        buffer, or `module.params` where the chain has none."""
        custom = self._native[self._index(module)].custom_weights()
        return module.params if custom is None else custom

    def state_dict(self):
        return {"hyperparams": self.hyperparams(), "modules": [{"n_params": opt.n, "snapshot": opt.serialize()} for opt in self._native]}

    def load_state_dict(self, state_dict):
        entries = state_dict["modules"]
        if len(entries) != len(self._native):
            raise ValueError("tinycudann.optim.Optimizer.load_state_dict: the state holds another number of modules")
        for opt, entry in zip(self._native, entries):
            if entry["n_params"] != opt.n:
                raise ValueError("tinycudann.optim.Optimizer.load_state_dict: a module has another number of parameters")
        self.update_hyperparams(state_dict["hyperparams"])
        for opt, entry in zip(self._native, entries):
            opt.deserialize(entry["snapshot"])
