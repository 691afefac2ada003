"""The fused GRU (csrc/rbx_gru.hip), the parts that need no GPU: the C ABI's entry points are declared, exported and bound, the
version stays put; refusals precede any launch; the gate answers on its edges; the float64 restatement of tests/gru64.py equals
torch.nn.GRU (packed sequences included) and reproduces the live reference's GRU4Rec and NARM
(tests/golden/rechub_session.npz, written by tests/gen_golden_session.py), which pins the restatement the GPU tests measure
against; the mirrors carry the reference's state_dict keys; the op refuses CPU tensors; the compat paths import."""
import ctypes
import importlib
import os
import re

import pytest
import torch
import torch.nn.utils.rnn as rnn_utils

import gru64
from conftest import Fixture, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_gru_supported", "rbx_gru_fwd", "rbx_gru_bwd"]
B, L, D, HID, V = 16, 6, 8, 12, 23
GRU_TOP = 128                                                # the top of the shipped range of hidden widths


def test_header_declares_the_entry_points_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)
    assert "gru4rec.py:40-44, 66-67" in text and "narm.py:30, 50-55" in text      # the entries cite what they replace


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rbx_version() == 124


def _fwd(lib, p, batch, seq_len, hidden, stride_t=None, dtype=2, len_dt=1):
    st = 3 * hidden if stride_t is None else stride_t
    return lib.rbx_gru_fwd(p, seq_len * max(st, 0), st, p, None, None, p, len_dt, batch, seq_len, hidden, dtype, p, p, p, None)


def _bwd(lib, p, batch, seq_len, hidden, stride_t=None, dtype=2, len_dt=1):
    st = hidden if stride_t is None else stride_t
    return lib.rbx_gru_bwd(p, p, p, seq_len * max(st, 0), st, p, p, len_dt, batch, seq_len, hidden, dtype, p, p, p, None)


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib = _lib.lib
    p = 0x1000                                               # fake, never dereferenced: every refusal precedes the launch
    assert _lib.RBX_F32 == 2 and _lib.RBX_I64 == 1
    for call in (_fwd, _bwd):
        for hidden in (6, 0, 132):
            assert call(lib, p, 4, 7, hidden) == _lib.RBX_ERR_UNSUPPORTED, hidden
            assert _lib.last_error()
        assert call(lib, p, 4, 0, 16) == _lib.RBX_ERR_UNSUPPORTED                          # seq_len = 0
        assert call(lib, p, 4, 7, 16, stride_t=50) == _lib.RBX_ERR_UNSUPPORTED             # a stride that is no multiple of 4
        assert call(lib, p, 4, 7, 16, dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED      # a float64 tensor code
        assert call(lib, p, 4, 7, 16, len_dt=_lib.RBX_F32) == _lib.RBX_ERR_UNSUPPORTED     # float lengths
        assert call(lib, p + 4, 4, 7, 16) == _lib.RBX_ERR_UNSUPPORTED                      # a misaligned base
        assert call(lib, p, 0, 7, 16) == _lib.RBX_OK                                       # empty batch


def test_gate_answers_on_its_edges():
    from recbox_amd import ops
    assert ops.GRU_MAX_HIDDEN == GRU_TOP
    assert ops.gru_supported(4, 1) and ops.gru_supported(64, 50) and ops.gru_supported(100, 20)
    assert ops.gru_supported(GRU_TOP, 200)
    assert not ops.gru_supported(GRU_TOP + 4, 50)
    assert not ops.gru_supported(0, 50) and not ops.gru_supported(6, 50) and not ops.gru_supported(62, 50)
    assert not ops.gru_supported(16, 0)


def test_op_refuses_cpu_tensors():
    from recbox_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gru(torch.randn(4, 7, 16), torch.randn(48, 16), torch.randn(48, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gru_torch(torch.randn(4, 7, 16), torch.randn(48, 16), torch.randn(48, 16))


def test_layer_mirrors_torch_gru_and_refuses_what_it_lacks():
    from recbox_amd.rechub.basic.layers import GRU
    for bias in (True, False):
        ours, ref = GRU(10, 12, num_layers=2, bias=bias, batch_first=True), torch.nn.GRU(10, 12, num_layers=2, bias=bias,
                                                                                          batch_first=True)
        assert list(ours.state_dict().keys()) == list(ref.state_dict().keys())
        for k, v in ref.state_dict().items():
            assert tuple(ours.state_dict()[k].shape) == tuple(v.shape), k
        ours.load_state_dict(ref.state_dict(), strict=True)
        for p in ours.parameters():
            assert p.abs().max() <= 1.0 / 12 ** 0.5
    for kw in ({"bidirectional": True}, {"dropout": 0.5}, {"proj_size": 4}):
        with pytest.raises(NotImplementedError):
            GRU(10, 12, **kw)


# ---- gru64 == torch.nn.GRU in float64 ---------------------------------------------------------------------------------------
def _torch_gru(I, H, layers, bias, seed):
    torch.manual_seed(seed)
    return torch.nn.GRU(I, H, num_layers=layers, bias=bias, batch_first=True).double()


def _grads(outs, leaves, ups):
    return torch.autograd.grad(sum((o * u).sum() for o, u in zip(outs, ups)), leaves, allow_unused=True)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("packed", [False, True])
def test_gru64_equals_torch_gru(layers, bias, packed):
    Bq, Lq, I, H = 9, 7, 5, 12
    ref = _torch_gru(I, H, layers, bias, 3)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(Bq, Lq, I, generator=g, dtype=torch.float64, requires_grad=True)
    h0 = torch.randn(layers, Bq, H, generator=g, dtype=torch.float64, requires_grad=True)
    up_o = torch.randn(Bq, Lq, H, generator=g, dtype=torch.float64)
    up_h = torch.randn(layers, Bq, H, generator=g, dtype=torch.float64)
    lengths = torch.tensor([7, 1, 3, 7, 2, 5, 4, 6, 1]) if packed else None
    if packed:
        pk = rnn_utils.pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)
        o, hn = ref(pk, h0)
        o, _ = rnn_utils.pad_packed_sequence(o, batch_first=True, total_length=Lq)
    else:
        o, hn = ref(x, h0)
    params = list(ref.parameters())
    want = _grads((o, hn), [x, h0] + params, (up_o, up_h))
    sd = dict(ref.named_parameters())
    o2, hn2 = gru64.gru(x, gru64.layers_of(sd, "", layers, bias), h0, lengths)
    got = _grads((o2, hn2), [x, h0] + params, (up_o, up_h))
    assert_close(o2, o, 1e-12, "out")
    assert_close(hn2, hn, 1e-12, "h_n")
    for name, a, b in zip(["dx", "dh0"] + [n for n, _ in ref.named_parameters()], got, want):
        assert_close(a, b, 1e-12, name)


def test_gru64_zero_length_gives_h0_and_a_zero_row():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 4, 5, generator=g, dtype=torch.float64)
    w_ih, w_hh = torch.randn(24, 5, generator=g, dtype=torch.float64), torch.randn(24, 8, generator=g, dtype=torch.float64)
    h0 = torch.randn(3, 8, generator=g, dtype=torch.float64)
    out, hn = gru64.gru_layer(x, w_ih, w_hh, None, None, h0, torch.tensor([0, 2, 4]))
    assert torch.equal(hn[0], h0[0]) and (out[0] == 0).all() and (out[1, 2:] == 0).all() and (out[2] != 0).all()


# ---- the fixture pins the restatement to the live reference -----------------------------------------------------------------
def _gru4rec64(fx):
    """(mode="user" output [B, D], y [B, D]) of GRU4Rec restated in float64 over gru64 (train mode: batch statistics)."""
    sd = {k: v.double() for k, v in fx.tensors("p_gru4rec").items()}
    x = fx.tensors("in")
    item = sd["embedding.embed_dict.item_id.weight"]
    h = gru64.gru4rec_history_state(sd, x["hist_item_id"], 2)
    inp = torch.cat([sd["embedding.embed_dict.user_id.weight"][x["user_id"]], h], dim=-1)
    z = inp @ sd["user_mlp.mlp.0.weight"].t() + sd["user_mlp.mlp.0.bias"]
    z = (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + 1e-5) * sd["user_mlp.mlp.1.weight"] + sd["user_mlp.mlp.1.bias"]
    user = torch.nn.functional.normalize(torch.relu(z), p=2, dim=-1)
    items = torch.nn.functional.normalize(torch.cat([item[x["item_id"]].unsqueeze(1), item[x["neg_items"]]], dim=1), p=2, dim=-1)
    return user, (user.unsqueeze(1) * items).sum(dim=1)


def test_float64_restatement_reproduces_the_reference_gru4rec():
    fx = Fixture("rechub_session")
    user, y = _gru4rec64(fx)
    assert tuple(fx["out_gru4rec"]["y"].shape) == (B, D)
    assert_close(user, fx["out_gru4rec"]["user"], 1e-6, "gru4rec user")
    assert_close(y, fx["out_gru4rec"]["y"], 1e-6, "gru4rec y")


def test_float64_restatement_reproduces_the_reference_narm():
    fx = Fixture("rechub_session")
    ids = fx.tensors("in")["session"]
    lengths = (ids != 0).sum(dim=1)
    assert lengths.min() == 1 and lengths.max() == L and set(lengths.tolist()) == set(range(1, L + 1))
    assert (ids != 0).long().cumsum(1).eq(torch.arange(1, L + 1)).eq(ids != 0).all()       # left-aligned
    sd = {k: v.double().requires_grad_() for k, v in fx.tensors("p_narm").items()}
    s = gru64.narm_scores(sd, ids)
    assert_close(s, fx["out_narm"]["s"], 1e-6, "narm s")
    # gradients of s.sum(): the reference computed them in fp32, so the bar scales with the gradient's size.  (The reference's
    # lookup gives its padding row no gradient; the restatement indexes the table, and a padded position reaches nothing.)
    names = list(sd.keys())
    grads = torch.autograd.grad(s.sum(), [sd[k] for k in names])
    for k, gk in zip(names, grads):
        ref = torch.from_numpy(fx["g_narm"][k]).double()
        assert_close(gk, ref, 1e-6 * max(1.0, ref.abs().max().item()), "narm grad " + k)


def _mirror(tag):
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.matching import GRU4Rec, NARM
    if tag == "narm":
        return NARM(SequenceFeature("session", vocab_size=V, embed_dim=D, pooling="concat"), HID, 0.0, 0.0)
    user = [SparseFeature("user_id", vocab_size=11, embed_dim=D)]
    hist = [SequenceFeature("hist_item_id", vocab_size=V, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", vocab_size=V, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=V, embed_dim=D, pooling="concat", shared_with="item_id")]
    return GRU4Rec(user, hist, item, neg, user_params={"dims": [D], "activation": "relu", "dropout": 0.0})


@pytest.mark.parametrize("tag", ["gru4rec", "narm"])
def test_mirrors_carry_the_reference_state_dict_keys(tag):
    fx = Fixture("rechub_session")
    model = _mirror(tag)
    assert set(model.state_dict().keys()) == set(fx["p_" + tag].keys())
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(fx["p_" + tag][k].shape), k
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    if tag == "narm":
        assert {"item_emb.weight", "a_1", "a_2", "v", "b", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0",
                "gru.bias_hh_l0"} == set(model.state_dict().keys())
    else:
        assert "gru.weight_hh_l1" in model.state_dict() and "gru.bias_ih_l0" not in model.state_dict()


def test_compat_names_the_models_and_their_paths_import():
    from recbox_amd import compat
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.matching.gru4rec"] == ("recbox_amd.rechub.models.matching", ["GRU4Rec"])
        assert table[root + ".models.matching.narm"] == ("recbox_amd.rechub.models.matching", ["NARM"])
        assert {"GRU4Rec", "NARM", "MIND", "ComirecDR", "DSSM", "YoutubeDNN", "SASRec"} <= set(table[root + ".models.matching"][1])
    report = compat.install(prefixes=("torch_rechub",), overlay=False)
    try:
        from recbox_amd.rechub.basic import layers as ours
        from recbox_amd.rechub.models import matching
        for path, name in (("torch_rechub.models.matching.gru4rec", "GRU4Rec"), ("torch_rechub.models.matching.narm", "NARM")):
            mod = importlib.import_module(path)
            if getattr(mod, "__recbox_amd__", False):
                assert getattr(mod, name) is getattr(matching, name)
        layers = importlib.import_module("torch_rechub.basic.layers")
        if getattr(layers, "__recbox_amd__", False):
            assert layers.GRU is ours.GRU
    finally:
        compat.uninstall(report)
