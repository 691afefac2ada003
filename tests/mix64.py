"""Float64 restatement of ``ops.expert_mix`` (csrc/rbx_mix.hip) with plain loops over gates and selections, forward and
backward written out (no autograd), plus the case builder and runner the tests share.  A helper, not a test module."""
import torch


def full_select(n_expert, n_gate):
    return [list(range(n_expert)) for _ in range(n_gate)]


def ple_select(n_task, n_specific, n_shared, with_shared_gate=True):
    """CGC's pattern: task i mixes its own experts and the shared ones; the last gate (below the top level) all of them."""
    n_all = n_task * n_specific + n_shared
    shared = list(range(n_task * n_specific, n_all))
    sel = [list(range(i * n_specific, (i + 1) * n_specific)) + shared for i in range(n_task)]
    if with_shared_gate:
        sel.append(list(range(n_all)))
    return sel


def make_case(seed, B, H, E, select, scale=1.0, up=1.0, x_scale=1.0):
    """{"x": E x [B, H] at std ``x_scale``, "z": T x [B, n_t] at std ``scale``, "up": T x [B, H] (upstream gradients at std
    ``up``), "select"} in float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return {"x": [torch.randn(B, H, generator=g) * x_scale for _ in range(E)],
            "z": [torch.randn(B, len(s), generator=g) * scale for s in select],
            "up": [torch.randn(B, H, generator=g) * up for _ in select],
            "select": [list(s) for s in select]}


def small_wrap_case(H, B=37):
    """The small-gradient case of tests/test_gpu_mix_forms.py and tests/test_fp32_bar_host.py: 16 experts, two gates over all
    of them (n_t = 16 > G at H = 8, 12, 32), expert outputs and logits of size 0.1, upstream gradients of size 1e-3 -- every
    dz is below 1e-4 there, where an absolute 1e-4 checks nothing."""
    return make_case(40 + H, B, H, 16, full_select(16, 2), scale=0.1, up=1e-3, x_scale=0.1)


def forward(x, z, select, softmax=True, dtype=torch.float64):
    """(outs, ps) in ``dtype``: float64 for the bound, float32 for the bar of tests/fp32_bar.py."""
    x = [t.to(dtype) for t in x]
    outs, ps = [], []
    for zt, sel in zip(z, select):
        zt = zt.to(dtype)
        if softmax:
            e = torch.exp(zt - zt.max(dim=1, keepdim=True).values)
            p = e / e.sum(dim=1, keepdim=True)
        else:
            p = zt
        out = torch.zeros_like(x[0])
        for j, e_idx in enumerate(sel):
            out = out + p[:, j:j + 1] * x[e_idx]
        outs.append(out)
        ps.append(p)
    return outs, ps


def backward(x, ps, select, douts, softmax=True, dtype=torch.float64, bug=None):
    """(dx: E tensors, dz: T tensors) in ``dtype``; an entry of ``douts`` may be None (no gradient = zeros).  ``bug``: one
    deliberately wrong term for tests/test_fp32_bar_host.py -- ("s_t over the first G entries", G): the sum s_t = sum_i p_i dp_i
    stops after G entries (a lane group of G lanes that does not wrap); "dz without - s_t"; "dX_e without the last gate"."""
    x = [t.to(dtype) for t in x]
    dx = [torch.zeros_like(t) for t in x]
    dz = []
    last_gate = {}
    for t, (sel, d) in enumerate(zip(select, douts)):
        if d is not None:
            for e_idx in sel:
                last_gate[e_idx] = t
    for t, (p, sel, d) in enumerate(zip(ps, select, douts)):
        if d is None:
            dz.append(torch.zeros_like(p))
            continue
        d = d.to(dtype)
        dp = torch.zeros_like(p)
        for j, e_idx in enumerate(sel):
            if not (bug == "dX_e without the last gate" and last_gate[e_idx] == t and t > 0):
                dx[e_idx] = dx[e_idx] + p[:, j:j + 1] * d
            dp[:, j] = (d * x[e_idx]).sum(dim=1)
        if not softmax:
            dz.append(dp)
            continue
        pd = p * dp
        if isinstance(bug, tuple) and bug[0] == "s_t over the first G entries":
            pd = pd[:, :bug[1]]
        s = pd.sum(dim=1, keepdim=True)
        dz.append(p * dp if bug == "dz without - s_t" else p * (dp - s))
    return dx, dz


def reference(case, softmax=True, used=None, dtype=torch.float64, bug=None):
    """{"out", "p", "dx", "dz"} of a case in ``dtype``; ``used``: the outputs that enter the loss (None = all)."""
    outs, ps = forward(case["x"], case["z"], case["select"], softmax, dtype)
    ups = [u if (used is None or t in used) else None for t, u in enumerate(case["up"])]
    dx, dz = backward(case["x"], ps, case["select"], ups, softmax, dtype, bug)
    return {"out": outs, "p": ps, "dx": dx, "dz": dz}


def reference32(case, softmax=True, used=None):
    """The same restatement in float32 on the CPU: the ``ref32`` of fp32_bar.assert_bar."""
    return reference(case, softmax, used, torch.float32)


def run(fn, case, device, softmax=True, used=None, grad_x=True, grad_z=True, x_override=None):
    """``fn(experts, gates, select, softmax)`` on ``device`` through autograd: {"out", "dx", "dz"} (None where no gradient was
    asked for).  ``x_override``: expert tensors to use instead of copies of ``case["x"]`` (views of a wider leaf, say); their
    gradients are then the caller's business (``dx`` is None)."""
    if x_override is None:
        x = [t.to(device).requires_grad_(grad_x) for t in case["x"]]
    else:
        x = list(x_override)
    z = [t.to(device).requires_grad_(grad_z) for t in case["z"]]
    outs = fn(x, z, case["select"], softmax)
    loss = sum((o * case["up"][t].to(device)).sum() for t, o in enumerate(outs) if used is None or t in used)
    leaves = (x if (grad_x and x_override is None) else []) + (z if grad_z else [])
    grads = list(torch.autograd.grad(loss, leaves, allow_unused=True)) if leaves else []
    n_x = len(x) if (grad_x and x_override is None) else 0
    return {"out": [o.detach() for o in outs], "loss": loss,
            "dx": grads[:n_x] if n_x else None, "dz": grads[n_x:] if grad_z else None}


# ---- the multi-task mirrors against the live reference's fixture (tests/golden/rechub_multi_task.npz) -----------------------
MODEL_NAMES = ("SharedBottom", "ESMM", "MMOE", "PLE", "AITM")


def mirror(tag):
    """This package's model ``tag``, built exactly as tests/gen_golden_multi_task.py builds the reference's."""
    import gen_golden_multi_task as gen
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import multi_task
    return gen.build(tag, features, {n: getattr(multi_task, n) for n in MODEL_NAMES})


def check_model_against_fixture(tag, device, tol=1e-4):
    """Load the fixture's parameters strictly, run forward + backward of y.sum() in train mode on ``device`` and compare y
    and every parameter gradient with what the reference recorded.  Returns the model."""
    from conftest import Fixture, assert_close, assert_grads_close
    fx = Fixture("rechub_multi_task")
    model = mirror(tag)
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][tag]]
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    model.to(device).train()
    y = model(fx.tensors("in", device))
    y.sum().backward()
    assert_close(y, fx["out_" + tag]["y"], tol, tag + " y")
    assert_grads_close(model, fx["g_" + tag], tol)
    return model
