"""Golden fixtures for class-conditional UNets: the three label embedding kinds the reference builds besides "sequential" (num_classes an
int, "continuous", "timestep") and ClassEmbedder trained through the loss.  Run from the repository root on a machine that has the reference
checkout:

    python -m tests.golden.make_golden_labels

Writes unet_labels_tiny_{int,continuous,timestep}.{safetensors,json} and class_engine_tiny.{safetensors,json} (data only).  The reference
runs in fp32 on bf16-exact inputs, with weights from synth_state_dict; x, context, timesteps and the upstream gradient of the UNet cases are
those of make_golden_adm.unet_inputs(), so its zero_gradient_noise() measures the analytically-zero gradients here as it does there."""
from __future__ import annotations

import torch

from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import FixedSigma, block_inputs, block_upstream, import_reference, synth_state_dict
from tests.golden.make_golden_adm import UNET_ADM_GRAD_KEYS, UNET_ADM_TINY, unet_inputs, zero_gradient_noise

LABEL_KINDS = {"int": 10, "continuous": "continuous", "timestep": "timestep"}
LABEL_Y = {
    "int": torch.tensor([3, 3]),                      # both samples hit one row
    "continuous": torch.tensor([[0.25], [-1.5]]),
    "timestep": torch.tensor([5.0, 700.0]),
}
CLASS_ENGINE = dict(embed_dim=48, n_classes=11, input_key="cls", is_trainable=True)
CLASS_IDS = [7, 2, 7, 10]
CLASS_SIGMAS = [0.8, 4.2, 0.3, 1.7]
CLASS_SHAPE = (4, 4, 16, 24)
CLASS_SEED = 515


def label_cfg(kind: str) -> dict:
    cfg = {k: v for k, v in UNET_ADM_TINY.items() if k != "adm_in_channels"}
    cfg["num_classes"] = LABEL_KINDS[kind]
    return cfg


def label_inputs(kind: str) -> dict:
    ins = unet_inputs()
    ins["y"] = LABEL_Y[kind].clone()
    return ins


def unet_labels_case(nd):
    for kind in LABEL_KINDS:
        cfg = label_cfg(kind)
        net = nd.UNetModel(**cfg).eval()
        shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict(synth_state_dict(shapes))
        ins = label_inputs(kind)
        if kind == "continuous":
            ins["y"].requires_grad_(True)
        out = net(ins["x"], ins["timesteps"], ins["context"], ins["y"])
        out.backward(block_upstream("unet_adm_tiny", out.shape))
        case = dict(cfg=cfg, shapes=shapes, F_out=out.detach().clone())
        case["grads"] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if k in UNET_ADM_GRAD_KEYS}
        case["label_grads"] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if k.startswith("label_emb.")}
        case["grad_norms"] = {k: float(p.grad.norm()) for k, p in net.named_parameters()}
        if kind == "continuous":
            case["d_y"] = ins["y"].grad.detach().clone()
            ins["y"] = ins["y"].detach()
        net.zero_grad()
        case["bf16_zero_grad_noise"] = zero_gradient_noise(net, ins, case["grad_norms"])
        save_fixture(case, f"unet_labels_tiny_{kind}")          # (one file per kind: each stays under the size limit of a committed file)
        print(f"labels unet {kind}: |out| {float(out.detach().abs().mean()):.4f} label keys {sorted(case['label_grads'])}")


def class_engine_inputs() -> dict:
    N, Cc, H, W = CLASS_SHAPE
    return block_inputs("class_engine_tiny", dict(x=(N, Cc, H, W), context=(N, 7, UNET_ADM_TINY["context_dim"])))


def class_engine_case(nd):
    from neurosis.modules.diffusion.loss import StandardDiffusionLoss
    from neurosis.modules.encoders import GeneralConditioner
    from neurosis.modules.encoders.classed import ClassEmbedder

    net = nd.UNetModel(**UNET_ADM_TINY).eval()
    ushapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(synth_state_dict(ushapes))
    emb = ClassEmbedder(**CLASS_ENGINE)
    eshapes = {k: list(v.shape) for k, v in emb.state_dict().items()}
    emb.load_state_dict(synth_state_dict(eshapes))
    conditioner = GeneralConditioner([emb])
    ins = class_engine_inputs()
    ids = torch.tensor(CLASS_IDS)
    sig = torch.tensor(CLASS_SIGMAS)
    denoiser = nd.DiscreteDenoiser(preconditioning=nd.EpsPreconditioning(), num_idx=1000, discretization=nd.LegacyDDPMDiscretization())
    loss_fn = StandardDiffusionLoss(sigma_generator=FixedSigma(sig), loss_weighting=nd.EpsWeighting(), loss_type="l2", objective_type="edm")
    # replay of the draws _forward makes, in its order, to record the noise it will use
    torch.manual_seed(CLASS_SEED)
    _t = torch.rand((CLASS_SHAPE[0],), dtype=torch.float64)
    noise = torch.randn_like(ins["x"])
    torch.manual_seed(CLASS_SEED)
    cond = conditioner({"cls": ids})
    assert list(cond) == ["vector"] and cond["vector"].requires_grad
    cond["crossattn"] = ins["context"]
    loss, extra = loss_fn._forward(nd.OpenAIWrapper(net), denoiser, cond, ins["x"], {}, return_dict=True)
    loss.mean().backward()
    assert torch.equal(extra["t"], _t)
    g = emb.embedding.weight.grad.detach().clone()
    hit = sorted(set(CLASS_IDS))
    assert all(float(g[v].abs().max()) > 0 for v in hit) and float(g[[v for v in range(CLASS_ENGINE["n_classes"]) if v not in hit]].abs().max()) == 0.0
    save_fixture(dict(unet_cfg=UNET_ADM_TINY, unet_shapes=ushapes, embedder=CLASS_ENGINE, embedder_shapes=eshapes, cls=ids, sigma=sig, noise=noise,
                      loss=loss.detach().clone(), d_embedding=g, seed=CLASS_SEED), "class_engine_tiny")
    print(f"class engine: loss {loss.tolist()} |d embedding| rows {[round(float(g[v].norm()), 5) for v in hit]}")


if __name__ == "__main__":
    torch.manual_seed(0)
    nd, _ = import_reference()
    unet_labels_case(nd)
    class_engine_case(nd)
