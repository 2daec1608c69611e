"""Highway layer (reference: common/Highway.py:5-37):  x <- sigma(G x) * f(N x) + (1 - sigma(G x)) * (L x).

The three Linears of a layer run as ONE GEMM over the row-concatenated weight [3*out, in]; the gate
arithmetic is a fused epilogue kernel (K14).  f must be tanh (the only value used in the reference)."""
import torch
import torch.nn as nn

from .. import ops, paramcache


class Highway(nn.Module):
    def __init__(self, input_size, output_size, num_layers=1, f=torch.tanh):
        super().__init__()
        if f is not torch.tanh:
            raise NotImplementedError("Highway on the HIP path implements f = tanh (the reference default)")
        self.num_layers = num_layers
        self.nonlinear = nn.ModuleList([nn.Linear(input_size, output_size) for _ in range(num_layers)])
        self.linear = nn.ModuleList([nn.Linear(input_size, output_size) for _ in range(num_layers)])
        self.gate = nn.ModuleList([nn.Linear(input_size, output_size) for _ in range(num_layers)])
        self.f = f

    def _pack(self, g, n, l):
        """gate | nonlinear | linear rows as one matrix.  Under autograd the concatenation is part of the graph (its backward hands
        each Linear its rows); without gradients (inference, the only place a layer is called many times per weight update) the
        packed f32 copy is kept in paramcache until a parameter moves (ops.linear casts it to bf16 on every call: caching that is a speed change)."""
        params = (g.weight, n.weight, l.weight, g.bias, n.bias, l.bias)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return torch.cat(params[:3], dim=0), torch.cat(params[3:], dim=0)
        return paramcache.derived(params, "highway", lambda: (torch.cat(params[:3], dim=0), torch.cat(params[3:], dim=0)))  # (no graph here)

    def forward(self, x):
        for n, l, g in zip(self.nonlinear, self.linear, self.gate):
            w, b = self._pack(g, n, l)  # [3*out, in]: gate | nonlinear | linear
            x = ops.highway_gate(ops.linear(x, w, b))
        return x
