"""float64 restatement of DCN-V2's mixture of low-rank cross experts (helper of tests/test_crossmix_host.py and
tests/test_gpu_crossmix.py, not a test).

``reference`` is the per-expert loop of the reference (rechub basic/layers.py, CrossNetMix) restated in plain torch -- matmuls
on [B, n, 1] columns, a stack into [B, n, E], a matmul with the softmax -- differentiated by autograd in float64 or, with
``dtype=torch.float32``, the same lines in fp32 on the CPU: the ``ref32`` of tests/fp32_bar.py.  It is not derived from
``ops.cross_mix_torch``.  The loss every test uses is ``sum(out * up)``; ``run`` evaluates it through the op under test and
returns the output and every gradient: dx0, per layer dU, dV, dC, db, and the shared dG.

``make_case`` scales V and C so that some tanh inputs exceed 3 in magnitude (the saturated branch) and most do not; it checks
both."""
import torch

MODELS = ("dcn", "v2par", "v2stk", "v2only", "edcn_h", "edcn_a", "wd")


def make_case(seed, B, n, E, r, L):
    g = torch.Generator().manual_seed(seed)
    case = {"x0": torch.randn(B, n, generator=g) * 0.8, "G": torch.randn(E, n, generator=g) * (1.0 / n ** 0.5),
            "U": [torch.randn(E, n, r, generator=g) * (0.6 / r ** 0.5) for _ in range(L)],
            "V": [torch.randn(E, n, r, generator=g) * (1.6 / n ** 0.5) for _ in range(L)],
            "C": [torch.randn(E, r, r, generator=g) * (1.8 / r ** 0.5) for _ in range(L)],
            "b": [torch.randn(n, 1, generator=g) * 0.2 for _ in range(L)],
            "up": torch.randn(B, n, generator=g), "dims": (B, n, E, r, L), "seed": seed}
    return case


def tanh_inputs(case):
    """Every value that enters a tanh, in float64, as one flat tensor."""
    seen = []
    reference(case, watch=seen)
    return torch.cat([t.reshape(-1) for t in seen])


def _forward(x0, U, V, C, G, b, watch=None):
    """rechub's CrossNetMix.forward with the parameters as arguments (``G`` [E, n]: the rows are the gates' weights)."""
    E = G.shape[0]
    x_0 = x0.unsqueeze(2)
    x_l = x_0
    for i in range(len(U)):
        outs, scores = [], []
        for e in range(E):
            scores.append(torch.matmul(x_l.squeeze(2), G[e:e + 1].t()))
            v_x = torch.matmul(V[i][e].t(), x_l)
            if watch is not None:
                watch.append(v_x.detach())
            v_x = torch.tanh(v_x)
            v_x = torch.matmul(C[i][e], v_x)
            if watch is not None:
                watch.append(v_x.detach())
            v_x = torch.tanh(v_x)
            uv_x = torch.matmul(U[i][e], v_x)
            outs.append((x_0 * (uv_x + b[i])).squeeze(2))
        outs = torch.stack(outs, 2)
        scores = torch.stack(scores, 1)
        x_l = torch.matmul(outs, scores.softmax(1)) + x_l
    return x_l.squeeze(2)


def names(L):
    out = ["out", "dx0", "dG"]
    for l in range(L):
        out += ["dU%d" % l, "dV%d" % l, "dC%d" % l, "db%d" % l]
    return out


def _collect(out, x0, G, U, V, C, b):
    res = {"out": out.detach(), "dx0": x0.grad, "dG": G.grad}
    for l in range(len(U)):
        res.update({"dU%d" % l: U[l].grad, "dV%d" % l: V[l].grad, "dC%d" % l: C[l].grad, "db%d" % l: b[l].grad})
    return res


def reference(case, dtype=torch.float64, watch=None):
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_()                 # noqa: E731
    x0, G = leaf(case["x0"]), leaf(case["G"])
    U, V, C, b = ([leaf(t) for t in case[k]] for k in ("U", "V", "C", "b"))
    out = _forward(x0, U, V, C, G, b, watch)
    (out * case["up"].to(dtype)).sum().backward()
    return _collect(out, x0, G, U, V, C, b)


def run(op, case, device, x0=None):
    """The same loss through ``op(x0, U_list, V_list, C_list, gate_w, bias_list)`` on ``device``; ``x0``: a prepared
    (view, leaf) pair to use instead of the case's x0."""
    leaf = lambda t: t.detach().clone().to(device).requires_grad_()                # noqa: E731
    G = leaf(case["G"])
    U, V, C, b = ([leaf(t) for t in case[k]] for k in ("U", "V", "C", "b"))
    if x0 is None:
        x = xleaf = leaf(case["x0"])
    else:
        x, xleaf = x0
    out = op(x, U, V, C, G, b)
    (out * case["up"].to(device)).sum().backward()
    return _collect(out, xleaf, G, U, V, C, b)


# ---- the mirrors against tests/golden/rechub_dcn.npz ---------------------------------------------------------------------------
def mirror(which):
    """This package's model ``which``, built exactly as tests/gen_golden_crossmix.py builds the reference's."""
    import gen_golden_crossmix as gen
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import ranking
    return gen.build(which, features, ranking)


def rel_err(got, want, scale=None):
    got, want = got.detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) if scale is None else scale
    return float((got - want).abs().max()) / max(scale, 1e-30)


def _next_module(model, param_name):
    """The module that follows the owner of ``param_name`` in its ``nn.Sequential`` (None if there is none)."""
    path = param_name.split(".")[:-1]
    parent = model.get_submodule(".".join(path[:-1]))
    if not isinstance(parent, torch.nn.Sequential) or not path[-1].isdigit() or int(path[-1]) + 1 >= len(parent):
        return None
    return parent[int(path[-1]) + 1]


def check_model_against_fixture(which, device, tol=1e-5):
    """Load the recorded parameters strictly, run forward + backward of y.sum() in train mode on ``device``; y and every
    parameter gradient within ``tol`` of the tensor's largest element.  As in tests/fibinet64.py, the bias of a Linear that feeds
    a train-mode BatchNorm has the exact gradient 0, so it is held to ``tol`` times the largest element of the recorded weight
    gradient of that Linear.  A gradient the reference recorded as all zero (EDCN's g1 / g2: a softmax over one element) must
    stay below ``tol`` outright.  Returns (model, y)."""
    from conftest import Fixture
    fx = Fixture("rechub_dcn")
    model = mirror(which)
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][which]]
    model.load_state_dict(fx.tensors("p_" + which), strict=True)
    model.to(device).train()
    y = model(fx.tensors("in", device))
    y.sum().backward()
    err = rel_err(y, fx["out_" + which]["y"])
    print("%s y: rel err %.3e" % (which, err))
    assert err <= tol, "%s y: %.3e" % (which, err)
    for name, p in model.named_parameters():
        want = fx["g_" + which][name]
        scale = None
        if name.endswith(".bias") and isinstance(_next_module(model, name), torch.nn.BatchNorm1d):
            scale = float(abs(fx["g_" + which][name[:-len("bias")] + "weight"]).max())
        elif float(abs(want).max()) == 0.0:
            scale = 1.0
        err = rel_err(p.grad if p.grad is not None else torch.zeros_like(p), want, scale)
        print("%s grad %s: rel err %.3e" % (which, name, err))
        assert err <= tol, "%s grad %s: %.3e" % (which, name, err)
    return model, y.detach()
