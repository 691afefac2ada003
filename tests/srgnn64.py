"""float64 restatement of one SR-GNN ``GNNCell`` and its gradients (helper of tests/test_srgnn_host.py and
tests/test_gpu_srgnn.py, not a test).  Per session, hidden X [L, H], A = [A_in | A_out] [L, 2 L]:

    I = [A_in (X W_ei^T + b_ei) + b_iah | A_out (X W_eo^T + b_eo) + b_ioh]      gi = I W_ih^T + b_ih      gh = X W_hh^T + b_hh
    r = sig(gi_r + gh_r)      z = sig(gi_z + gh_z)      n = tanh(gi_n + r gh_n)      hy = (1 - z) X + z n

``forward`` states this row by row with explicit sums over the neighbours and the gates written out, in a chosen dtype on
the CPU, so it shares no code with ``ops.session_gnn_step_torch``.  ``reference`` is that in float64 with its gradients of
``sum(hy * up)``; ``ref32`` the same in float32 (the ``ref32`` of tests/fp32_bar.py); ``run`` evaluates the loss through the
op under test.  ``A`` gets no gradient.

``make_case`` draws Gaussians: hidden and up standard, the matrices with deviation 1 / sqrt(fan-in), the biases times 0.5.
``A`` comes from ``ops.session_graph_torch`` of random sessions over a vocabulary of 7 (``dense=False``) or is a random
non-negative dense matrix (``dense=True``): the cell takes any A.  The gates are smooth, so no seed is screened."""
import math

import torch

WEIGHTS = ("w_edge_in", "b_edge_in", "w_edge_out", "b_edge_out", "b_iah", "b_ioh", "w_ih", "w_hh", "b_ih", "b_hh")
GRADS = ("dhidden",) + tuple("d" + n for n in WEIGHTS)
NAMES = ("hy",) + GRADS


def forward(A, hidden, w_edge_in, b_edge_in, w_edge_out, b_edge_out, b_iah, b_ioh, w_ih, w_hh, b_ih, b_hh):
    """hy [B, L, H] in the dtype of the tensors."""
    B, L, H = hidden.shape
    e_in = torch.einsum("blk,nk->bln", hidden, w_edge_in) + b_edge_in
    e_out = torch.einsum("blk,nk->bln", hidden, w_edge_out) + b_edge_out
    a_in = (A[:, :, :L].unsqueeze(-1) * e_in.unsqueeze(1)).sum(2) + b_iah          # [B, i, j, 1] * [B, 1, j, H] over j
    a_out = (A[:, :, L:].unsqueeze(-1) * e_out.unsqueeze(1)).sum(2) + b_ioh
    gi = torch.einsum("blk,nk->bln", a_in, w_ih[:, :H]) + torch.einsum("blk,nk->bln", a_out, w_ih[:, H:]) + b_ih
    gh = torch.einsum("blk,nk->bln", hidden, w_hh) + b_hh
    r = 1.0 / (1.0 + torch.exp(-(gi[..., :H] + gh[..., :H])))
    z = 1.0 / (1.0 + torch.exp(-(gi[..., H:2 * H] + gh[..., H:2 * H])))
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return hidden - z * hidden + z * n


def make_case(B, L, H, seed=0, dense=False):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(100003 * seed + 1009 * B + 31 * L + 7 * H + int(dense))
    if dense:
        A = torch.rand(B, L, 2 * L, generator=g) * (torch.rand(B, L, 2 * L, generator=g) < 0.5)
    else:
        lengths = torch.randint(0, L + 1, (B,), generator=g)
        seq = torch.randint(1, 8, (B, L), generator=g) * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
        A = ops.session_graph_torch(seq)[1]
    return {"dims": (B, L, H), "A": A.float(),
            "hidden": torch.randn(B, L, H, generator=g),
            "w_edge_in": torch.randn(H, H, generator=g) / math.sqrt(H), "b_edge_in": torch.randn(H, generator=g) * 0.5,
            "w_edge_out": torch.randn(H, H, generator=g) / math.sqrt(H), "b_edge_out": torch.randn(H, generator=g) * 0.5,
            "b_iah": torch.randn(H, generator=g) * 0.5, "b_ioh": torch.randn(H, generator=g) * 0.5,
            "w_ih": torch.randn(3 * H, 2 * H, generator=g) / math.sqrt(2 * H),
            "w_hh": torch.randn(3 * H, H, generator=g) / math.sqrt(H),
            "b_ih": torch.randn(3 * H, generator=g) * 0.5, "b_hh": torch.randn(3 * H, generator=g) * 0.5,
            "up": torch.randn(B, L, H, generator=g)}


def run(fn, case, device, needs=None, dtype=None, hidden_of=None):
    """The loss ``sum(hy * up)`` through ``fn(A, hidden, *weights) -> hy`` on ``device``.  ``needs``: which of (hidden,) +
    WEIGHTS require a gradient (default all).  ``hidden_of``: maps the hidden leaf to what the op is given (a view of it).
    Returns {"hy", "dhidden", "dw_edge_in", ...}."""
    needs = (True,) * 11 if needs is None else needs
    names = ("hidden",) + WEIGHTS

    def put(t):
        t = t.detach().clone().to(device)
        return t.to(dtype) if dtype is not None else t
    t = {n: put(case[n]).requires_grad_(needs[i]) for i, n in enumerate(names)}
    A, up = put(case["A"]), put(case["up"])
    hidden = t["hidden"] if hidden_of is None else hidden_of(t["hidden"])
    hy = fn(A, hidden, *[t[n] for n in WEIGHTS])
    if any(needs):
        (hy * up).sum().backward()
    out = {"hy": hy.detach()}
    for n in names:
        out["d" + n] = t[n].grad
    return out


def reference(case):
    """The dict of ``run`` in float64 on the CPU through ``forward``."""
    return run(forward, case, "cpu", dtype=torch.float64)


def ref32(case):
    """The same in float32 with plain torch ops on the CPU."""
    return run(forward, case, "cpu", dtype=torch.float32)
