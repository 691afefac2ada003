"""Self-attentive multi-interest pooling on the GPU (``ops.sa_pool``, the einsum composition of the reference's lines) against
the float64 restatement of tests/sa64.py at the project's absolute 1e-4, and ComirecSA / SINE against the live reference's
fixture.  Shapes (L, D, H, K): one row per sample, short and long sequences, D = 128 with H = 512, K = 1 and K = 32, H that is
not 4 D and not a power of two."""
import importlib

import pytest
import torch

import sa64
from conftest import Fixture, assert_close
from test_sa_host import check_model_against_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("out", "attn", "dx", "dw1", "dw2")
SHAPES = [(1, 16, 64, 4), (7, 16, 64, 4), (50, 64, 256, 4), (200, 64, 256, 4), (50, 128, 512, 8), (20, 32, 128, 1), (64, 4, 16, 2),
          (33, 20, 80, 3), (65, 8, 32, 32), (9, 96, 384, 2), (12, 16, 20, 2), (12, 32, 100, 3)]
_REF = {}


def ops():
    from recbox_amd import ops as o
    return o


def case_and_reference(B, shape, **kw):
    key = (B, shape, tuple(sorted(kw.items())))
    if key not in _REF:
        case = sa64.make_case(B, *shape)
        _REF[key] = (case, sa64.reference(case, **kw))
    return _REF[key]


def compare(got, want, what, names=NAMES):
    for n in names:
        assert_close(got[n], want[n], 1e-4, "%s %s" % (what, n))


@pytest.mark.parametrize("B", [37, 301])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float64_comparison_over_shapes(B, shape):
    case, want = case_and_reference(B, shape)
    compare(sa64.run(ops().sa_pool, case, DEV), want, "sa_pool")


@pytest.mark.parametrize("shape", [(7, 16, 64, 4), (50, 64, 256, 4)], ids=lambda s: "x".join(map(str, s)))
def test_output_and_gradient_forms(shape):
    o = ops()
    for kw in ({"use_attn": False}, {"use_out": False}):
        case, want = case_and_reference(37, shape, **kw)
        compare(sa64.run(o.sa_pool, case, DEV, **kw), want, "sa_pool %s" % sorted(kw))
    case, want = case_and_reference(37, shape, use_out=False)
    x, w1, w2 = (case[n].to(DEV).requires_grad_(True) for n in ("x", "w1", "w2"))
    out, attn = o.sa_pool(x, w1, w2, case["mask"].to(DEV), pool=False)
    assert out is None
    assert_close(attn, want["attn"], 1e-4, "pool=False attn")
    grads = torch.autograd.grad((attn * case["g_attn"].to(DEV)).sum(), (x, w1, w2))
    for g, n in zip(grads, ("dx", "dw1", "dw2")):
        assert_close(g, want[n], 1e-4, "pool=False " + n)


def test_masks():
    o = ops()
    shape = (7, 16, 64, 4)
    case, want = case_and_reference(37, shape)
    L = shape[0]
    got = sa64.run(o.sa_pool, case, DEV)
    mask = case["mask"]
    assert int(mask[0].sum()) == 0                                              # sample 0 is fully masked
    assert torch.equal(got["attn"][0].cpu(), torch.full((L, 4), 1.0 / L))       # exactly 1 / L
    assert_close(got["out"][0], case["x"][0].mean(dim=0).expand(4, -1), 1e-6, "fully masked out = row mean")
    assert float(got["dx"][0].abs().max()) > 0.0                                # ... and it carries gradient: no mask factor
    assert_close(got["dx"][0], want["dx"][0], 1e-4, "fully masked dx")
    partly = (mask.sum(1) > 0) & (mask.sum(1) < L)
    assert bool(partly.any())
    gone = (mask == 0) & partly.unsqueeze(1)
    assert float(got["attn"].cpu()[gone].abs().max()) == 0.0                    # masked positions of a partly masked sample
    for other in (mask.int(), mask.float(), mask.bool(), mask.float().unsqueeze(-1)):
        again = sa64.run(o.sa_pool, case, DEV, mask=other.to(DEV))
        for n in NAMES:
            assert torch.equal(again[n], got[n]), (other.dtype, n)
    free, want_free = sa64.run(o.sa_pool, case, DEV, masked=False), sa64.reference(case, masked=False)
    compare(free, want_free, "mask=None")


def test_large_logits_as_written():
    """A fully masked sample whose logits are exactly +-40 and +-100: the fp32 sum with -1e9 keeps them as multiples of 64
    (-1e9 + 64 / - 64, -1e9 + 128 / - 128), so both interests put 1/2 on positions 0 and 2 -- not 1/4 everywhere."""
    o = ops()
    x = torch.tensor([1.0, -1.0, 1.0, -1.0]).reshape(1, 4, 1) * 10.0 * torch.ones(1, 4, 4)
    w1 = torch.ones(4, 64)
    w2 = torch.stack([torch.full((64,), 40.0 / 64), torch.full((64,), 100.0 / 64)], dim=1)
    mask = torch.zeros(1, 4, dtype=torch.long)
    out_c, attn_c = o.sa_pool_torch(x, w1, w2, mask)                            # fp32 on the CPU
    out_g, attn_g = o.sa_pool(x.to(DEV), w1.to(DEV), w2.to(DEV), mask.to(DEV))
    literal = torch.tensor([0.5, 0.0, 0.5, 0.0]).reshape(1, 4, 1).expand(1, 4, 2)
    assert torch.equal(attn_c, literal) and torch.equal(attn_g.cpu(), literal)
    assert torch.equal(out_g.cpu(), out_c) and torch.equal(out_c, torch.full((1, 2, 4), 10.0))


@pytest.mark.parametrize("tag", ["comirec_sa", "sine"])
def test_models_match_the_reference(tag):
    model = check_model_against_fixture(tag, DEV)
    if tag == "comirec_sa":
        g3 = model.multi_interest_sa.W3.grad
        assert g3 is None or float(g3.abs().max()) == 0.0


def test_compat_paths_resolve():
    from recbox_amd import compat
    from recbox_amd.rechub.basic import layers as ours
    from recbox_amd.rechub.models import matching
    report = compat.install(prefixes=("torch_rechub",), overlay=True)
    try:
        assert importlib.import_module("torch_rechub.models.matching.comirec").ComirecSA is matching.ComirecSA
        assert importlib.import_module("torch_rechub.models.matching.sine").SINE is matching.SINE
        assert importlib.import_module("torch_rechub.basic.layers").MultiInterestSA is ours.MultiInterestSA
    finally:
        compat.uninstall(report)
