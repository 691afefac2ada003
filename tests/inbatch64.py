"""float64 restatement of the in-batch band scores (helper of tests/test_inbatch_host.py and tests/test_gpu_inbatch.py, not a
test).

``reference`` states the band directly -- with j = (i + k) mod B

    scores[i, k] = (<u_i, v_j> / (max(|u_i|, eps) max(|v_j|, eps)) - log w_j) / temperature

-- in plain torch, a Python loop over k, differentiated by autograd in float64 or, with ``dtype=torch.float32``, the same lines
in fp32 on the CPU: the ``ref32`` of tests/fp32_bar.py.  A norm under ``eps`` is clamped by ``clamp_min``, whose derivative is
zero there: a constant denominator.  It is not derived from ``ops.inbatch_band_scores_torch``.  ``literal`` is the reference
model's own expression (``torch.cosine_similarity`` broadcast to [B, B, D], ``- log w``, ``[index0, index1]``, ``/ temperature``).
The loss every test uses is ``sum(scores * g)`` with a seeded ``g``; ``run`` evaluates it through the op under test and returns
scores, du, dv and dw.

``make_case`` draws the weights from [0.05, 1]."""
import numpy as np
import torch

NAMES = ("scores", "du", "dv", "dw")
EPS = 1e-8


def make_case(seed, B, D, n_neg, weighted, temperature=0.5):
    g = torch.Generator().manual_seed(seed)
    case = {"u": torch.randn(B, D, generator=g), "v": torch.randn(B, D, generator=g) * 1.5,
            "w": 0.05 + 0.95 * torch.rand(B, generator=g) if weighted else None,
            "g": torch.randn(B, n_neg + 1, generator=g), "n_neg": n_neg, "temperature": temperature, "dims": (B, D, n_neg),
            "seed": seed}
    return case


def names(case):
    return NAMES if case["w"] is not None else NAMES[:3]


def _band(u, v, w, n_neg, temperature, eps=EPS):
    B = u.shape[0]
    nu, nv = u.norm(dim=1).clamp_min(eps), v.norm(dim=1).clamp_min(eps)
    cols = []
    for k in range(n_neg + 1):
        j = (torch.arange(B) + k) % B
        s = (u * v[j]).sum(1) / (nu * nv[j])
        if w is not None:
            s = s - torch.log(w[j])
        cols.append(s / temperature)
    return torch.stack(cols, 1)


def _collect(scores, u, v, w):
    res = {"scores": scores.detach(), "du": u.grad, "dv": v.grad}
    if w is not None:
        res["dw"] = w.grad
    return res


def reference(case, dtype=torch.float64):
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_()                 # noqa: E731
    u, v = leaf(case["u"]), leaf(case["v"])
    w = leaf(case["w"]) if case["w"] is not None else None
    scores = _band(u, v, w, case["n_neg"], case["temperature"])
    (scores * case["g"].to(dtype)).sum().backward()
    return _collect(scores, u, v, w)


def literal(case, dtype=torch.float64):
    """The scores as rechub's YoutubeSBC.forward writes them, on a full batch."""
    B, n = case["u"].shape[0], case["n_neg"]
    u, v = case["u"].to(dtype), case["v"].to(dtype)
    index0 = np.repeat(np.arange(B), n + 1)
    index1 = np.concatenate([np.arange(i, i + n + 1) for i in range(B)])
    index1[np.where(index1 >= B)] -= B
    pred = torch.cosine_similarity(u.unsqueeze(1), v, dim=2)
    scores = pred - torch.log(case["w"].to(dtype)) if case["w"] is not None else pred
    scores = scores[index0, index1] / case["temperature"]
    return scores.view(-1, n + 1)


def run(op, case, device, u=None, v=None):
    """The same loss through ``op(u, v, n_neg, weight=, temperature=)`` on ``device``; ``u`` / ``v``: a prepared (view, leaf)
    pair to use instead of the case's tensor."""
    leaf = lambda t: t.detach().clone().to(device).requires_grad_()                # noqa: E731
    uu, uleaf = u if u is not None else (leaf(case["u"]),) * 2
    vv, vleaf = v if v is not None else (leaf(case["v"]),) * 2
    w = leaf(case["w"]) if case["w"] is not None else None
    scores = op(uu, vv, case["n_neg"], weight=w, temperature=case["temperature"])
    (scores * case["g"].to(device=device, dtype=scores.dtype)).sum().backward()
    return _collect(scores, uleaf, vleaf, w)


# ---- the mirrors against tests/golden/rechub_inbatch.npz -----------------------------------------------------------------------
def mirror(which):
    """This package's model ``which`` ('sbc' / 'fb'), built exactly as tests/gen_golden_inbatch.py builds the reference's."""
    import gen_golden_inbatch as gen
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import matching
    return gen.build(which, features, matching)


def rel_err(got, want, scale=None):
    got, want = got.detach().double().cpu(), torch.as_tensor(np.asarray(want)).double()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) if scale is None else scale
    return float((got - want).abs().max()) / max(scale, 1e-30)


def grad_scale(model, name, recorded):
    """None (the tensor's own largest element) except, as in tests/crossmix64.py, for the bias of a Linear that feeds a
    train-mode BatchNorm: its exact gradient is 0, so it is held against the largest element of the recorded weight gradient
    of that Linear."""
    path = name.split(".")[:-1]
    parent = model.get_submodule(".".join(path[:-1]))
    if (name.endswith(".bias") and isinstance(parent, torch.nn.Sequential) and path[-1].isdigit() and int(path[-1]) + 1 < len(parent)
            and isinstance(parent[int(path[-1]) + 1], torch.nn.BatchNorm1d)):
        return float(np.abs(recorded[name[:-len("bias")] + "weight"]).max())
    return None


def loaded(which, device):
    from conftest import Fixture
    fx = Fixture("rechub_inbatch")
    model = mirror(which)
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][which]]
    model.load_state_dict(fx.tensors("p_" + which), strict=True)
    return model.to(device).train(), fx


def step(which, model, fx, tag, device):
    """Forward + backward of the recorded loss on the recorded batch ``tag`` ('full' / 'short' for sbc, 'full' for fb): returns
    ({output name: tensor}, {parameter: gradient})."""
    import gen_golden_inbatch as gen
    model.zero_grad()
    x = fx.tensors("in_%s_%s" % (which, tag), device)
    outs = gen.outputs(which, model(x))
    gen.loss(which, outs, fx.tensors("up_%s_%s" % (which, tag), device)).backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for n, p in model.named_parameters()}
    return {k: t.detach() for k, t in outs.items()}, grads
