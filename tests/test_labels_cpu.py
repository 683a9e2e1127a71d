"""Class-conditional UNets and ClassEmbedder without a GPU: the constructors' module trees against the reference's state-dict keys
(tests/golden/make_golden_labels.py), the class paths under the prefix swap, the unconditional class, and the refusals by name."""
import importlib

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden import synth_state_dict
from tests.golden.make_golden_labels import LABEL_KINDS, label_cfg

LABEL_KEYS = {
    "int": {"label_emb.weight": [10, 128]},
    "continuous": {"label_emb.weight": [128, 1], "label_emb.bias": [128]},
    "timestep": {"label_emb.1.0.weight": [128, 32], "label_emb.1.0.bias": [128], "label_emb.1.2.weight": [128, 128], "label_emb.1.2.bias": [128]},
}


def _resolve(path):
    module, _, cls = path.replace("neurosis.", "neurosis_amd.", 1).rpartition(".")
    return getattr(importlib.import_module(module), cls)


@pytest.mark.parametrize("kind", list(LABEL_KINDS))
def test_constructor_keys_and_shapes_are_the_references(kind):
    import neurosis_amd.modules.diffusion as D

    fx = load_fixture(f"unet_labels_tiny_{kind}")
    assert fx["cfg"] == label_cfg(kind) and "adm_in_channels" not in fx["cfg"]
    net = D.UNetModel(**fx["cfg"])
    mine = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert mine == fx["shapes"]
    assert {k: v for k, v in mine.items() if k.startswith("label_emb.")} == LABEL_KEYS[kind]
    res = net.load_state_dict(synth_state_dict(fx["shapes"]), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(fx["label_grads"]) == sorted(LABEL_KEYS[kind])


def test_sequential_and_none_are_unchanged_and_an_unknown_kind_is_refused():
    import neurosis_amd.modules.diffusion as D

    fx = load_fixture("unet_labels_tiny_int")
    base = {k: v for k, v in fx["cfg"].items() if k != "num_classes"}
    assert not any(k.startswith("label_emb") for k in D.UNetModel(**base).state_dict())
    seq = D.UNetModel(**base, num_classes="sequential", adm_in_channels=48).state_dict()
    assert sorted(k for k in seq if k.startswith("label_emb")) == ["label_emb.0.0.bias", "label_emb.0.0.weight", "label_emb.0.2.bias", "label_emb.0.2.weight"]
    for bad in ("classes", "Continuous", 2.5):
        with pytest.raises(NotImplementedError, match="num_classes"):
            D.UNetModel(**base, num_classes=bad)


def test_class_embedder_paths_and_unconditional_class():
    from neurosis_amd.modules.encoders.classed import ClassEmbedder

    assert _resolve("neurosis.modules.encoders.ClassEmbedder") is ClassEmbedder
    assert _resolve("neurosis.modules.encoders.classed.ClassEmbedder") is ClassEmbedder
    emb = ClassEmbedder(embed_dim=48, n_classes=11, input_key="cls")
    assert {k: list(v.shape) for k, v in emb.state_dict().items()} == {"embedding.weight": [11, 48]}
    assert not emb.is_trainable and emb.ucg_rate == 0.0 and emb.add_sequence_dim is False
    uc = emb.get_unconditional_conditioning(3, device="cpu")
    assert list(uc) == ["cls"] and uc["cls"].dtype == torch.int64 and uc["cls"].tolist() == [10, 10, 10]
    tr = ClassEmbedder(embed_dim=48, n_classes=11, input_key="cls", is_trainable=True, add_sequence_dim=True)
    assert tr.is_trainable and tr.add_sequence_dim and len(tr.trained_parameters()) == 1 and tr.trained_parameters()[0] is tr.embedding.weight
    fx = load_fixture("class_engine_tiny")
    assert fx["embedder_shapes"] == {"embedding.weight": [11, 48]}
    assert not hasattr(importlib.import_module("neurosis_amd.modules.encoders.classed"), "ClassEmbedderForMultiCond")


def test_cpu_tensors_have_no_path():
    from neurosis_amd import ops
    from neurosis_amd.modules.encoders import ClassEmbedder

    table = torch.nn.Parameter(torch.zeros(10, 16))
    ids = torch.tensor([1, 2])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.label_rows(table, ids)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.label_rows_bwd(ids, torch.zeros(2, 16), table)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.linear1_fwd(torch.zeros(2, 1), torch.nn.Parameter(torch.zeros(16, 1)), torch.nn.Parameter(torch.zeros(16)))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ClassEmbedder(embed_dim=16, n_classes=10, input_key="cls")(ids)


def test_y_is_validated_by_name():
    import neurosis_amd.modules.diffusion as D

    x, t, ctx = torch.zeros(2, 4, 16, 24), torch.tensor([1, 2]), torch.zeros(2, 7, 64)
    net = D.UNetModel(**label_cfg("int"))
    with pytest.raises(ValueError, match=r"int64 class ids of shape \[B\]"):
        net(x, t, ctx, torch.tensor([3.0, 3.0]))
    with pytest.raises(ValueError, match=r"int64 class ids of shape \[B\]"):
        net.label_input(torch.tensor([[3], [3]]))
    net = D.UNetModel(**label_cfg("continuous"))
    with pytest.raises(ValueError, match=r"float tensor of shape \[B, 1\]"):
        net(x, t, ctx, torch.tensor([0.25, -1.5]))
    with pytest.raises(ValueError, match=r"float tensor of shape \[B, 1\]"):
        net.label_input(torch.tensor([[1], [2]]))
    net = D.UNetModel(**label_cfg("timestep"))
    with pytest.raises(ValueError, match=r"float tensor of shape \[B\]"):
        net(x, t, ctx, torch.tensor([[5.0], [700.0]]))
    # the accepted forms come back in the chain's own form without a launch
    assert net.label_input(torch.tensor([5.0, 700.0], dtype=torch.float64)).dtype == torch.float32
    ids = torch.tensor([3, 3])
    assert D.UNetModel(**label_cfg("int")).label_input(ids) is ids
