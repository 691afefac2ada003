"""SR-GNN's mirrors on the GPU (recbole.SRGNNEncoder, rechub's SRGNN): the session graph built on the device with the bits of
the CPU run, the encoder against tests/golden/srgnn.npz (recorded from the live reference by tests/gen_golden_srgnn.py) at the
project's fixture bar, 1e-4 on outputs and gradients.  The lookup, the Linears and the catalogue product are the library's
kernels; the graph and the cell are ATen (ops.session_graph_torch, ops.session_gnn_step_torch)."""
import pytest
import torch

import fp32_bar
import srgnn64 as sg
from conftest import Fixture

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,L", [(1, 1), (37, 2), (37, 17), (301, 50), (5, 65)])
def test_session_graph_on_the_device_has_the_cpu_bits(B, L):
    """Ids from a vocabulary of 7 (0 included), so repeats, self-loops and early zeros are dense; also the fixture's sessions."""
    from recbox_amd import ops
    seq = torch.randint(0, 7, (B, L), generator=torch.Generator().manual_seed(31 * B + L))
    fx = Fixture("srgnn").tensors("graph")
    for s, want in ((seq, ops.session_graph_torch(seq)), (fx["seq"], (fx["alias"], fx["A"], fx["items"], fx["seq"] > 0))):
        got = ops.session_graph_torch(s.cuda())
        for name, a, b in zip(("alias", "A", "items", "mask"), got, want):
            assert a.dtype == b.dtype and a.is_cuda, name
            assert torch.equal(a.cpu().view(torch.int32) if name == "A" else a.cpu(), b.view(torch.int32) if name == "A" else b), name


@pytest.mark.parametrize("B,L,H,dense", [(37, 5, 12, False), (37, 17, 16, True), (7, 20, 100, False)])
def test_cell_on_the_device_against_float64(B, L, H, dense):
    from recbox_amd import ops
    case = sg.make_case(B, L, H, 0, dense)
    want, ref32 = sg.reference(case), sg.ref32(case)
    got = sg.run(ops.session_gnn_step_torch, case, "cuda")
    for n in sg.NAMES:
        fp32_bar.assert_bar("%s L%d H%d" % (n, L, H), got[n], want[n], ref32[n])


@pytest.mark.parametrize("c", [0, 1, 2])
def test_encoder_against_the_reference_fixture(c):
    from test_srgnn_host import check_encoder
    check_encoder(c, "cuda")


def test_rechub_model_against_the_fixture_and_an_empty_session():
    from recbox_amd.rechub.basic.features import SequenceFeature
    from recbox_amd.rechub.models.matching import SRGNN
    from test_srgnn_host import CASES
    fx = Fixture("srgnn")
    B, L, H, step, n_items = CASES[0]
    model = SRGNN(SequenceFeature("hist", vocab_size=n_items, embed_dim=H, pooling="concat"), step=step)
    model.encoder.load_state_dict(fx.tensors("p0"), strict=True)
    model.cuda().train()
    seq = fx.tensors("in0", "cuda")["seq"]
    scores = model({"hist": seq})
    want = torch.from_numpy(fx["out0"]["seq_output"]).double() @ model.encoder.item_embedding.weight.detach().double().cpu().t()
    err = float((scores.detach().double().cpu() - want).abs().max())
    assert tuple(scores.shape) == (B, n_items) and err <= 1e-4, err
    scores.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    seq = seq.clone()
    seq[5] = 0                                                          # an empty session
    out = model({"hist": seq})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    keep = [i for i in range(B) if i != 5]
    assert float((out[keep] - scores[keep]).detach().abs().max()) <= 1e-5
