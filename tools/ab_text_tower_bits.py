"""Bits and launch sequences of the text towers (models/text_encoder: CLIP-L in the HuggingFace layout, OpenCLIP, T5 / ByT5) under two source
trees: each tree runs the same tiny towers in a fresh child process of its own (--root selects the tree the child imports), which prints

    ROW   <case> <tensor> <sha256>      every frozen output, every trained output and every trained parameter's gradient after one micro-batch
                                        in overwrite mode and after a second one in accumulate mode
    CALL  <case> <entry point and its integer / float arguments>      the steady state: the second forward (+ backward) with unchanged parameters
    FIRST <case> <entry point>          the first forward (+ backward), which also builds the bf16 copies

and the parent compares them line for line.  Only names both trees have are used: the tower and embedder classes, forward, train_outputs.
ROW and CALL lines must be identical (exit status 0 only then); FIRST lines may differ, and the difference is listed per entry point.

    python tools/ab_text_tower_bits.py --a PARENT_TREE --b . --label-a COMMIT --label-b COMMIT --out profiles/text_towers_refactor_bits.txt

Each child runs under its own time limit; if the first one fails or runs out of time the second is not started."""
from __future__ import annotations

import argparse
import collections
import hashlib
import subprocess
import sys
from pathlib import Path

HF = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2)
OPEN_CLIP = dict(vocab_size=512, width=128, layers=3, heads=2, embed_dim=64)
T5 = dict(vocab_size=384, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=3, relative_attention_num_buckets=32)
T5_LENGTHS = (24, 40)


def child() -> None:
    import ctypes

    import torch

    import neurosis_amd.lib as lib
    from neurosis_amd.models.text_encoder import (CLIPTextTower, FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2, OpenCLIPTextTower, T5EncoderTower)
    from neurosis_amd.nn import FlatParamStore

    log = None
    real_call = lib.call

    def scalars(args):
        out = []
        for a in args:
            a = getattr(a, "_obj", a)      # byref(struct) -> the struct
            if isinstance(a, ctypes.Structure):
                out.append("{" + " ".join(scalars([getattr(a, f) for f, _ in a._fields_])) + "}")
            elif isinstance(a, bool) or (isinstance(a, int) and abs(a) < 1 << 32):      # (larger integers are addresses)
                out.append(str(int(a)))
            elif isinstance(a, float):
                out.append(repr(a))
        return out

    def recording_call(name, *args):
        if log is not None:
            log.append(name + " " + " ".join(scalars(args)))
        return real_call(name, *args)

    lib.call = recording_call
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("neurosis_amd") and getattr(mod, "call", None) is real_call:
            mod.call = recording_call

    def emit(case, **outs):
        torch.cuda.synchronize()
        for k, t in outs.items():
            raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
            print(f"ROW {case} {k} {hashlib.sha256(raw).hexdigest()}", flush=True)

    def recorded(case, kind, fn):
        nonlocal log
        log = []
        out = fn()
        torch.cuda.synchronize()
        for line in log:
            print(f"{kind} {case} {line if kind == 'CALL' else line.split(' ')[0]}", flush=True)
        log = None
        return out

    def randomize(module, seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in module.named_parameters():
                if p.dim() == 0:
                    continue
                if p.dim() == 1:
                    p.copy_((1.0 if "norm" in name or "ln_" in name else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * (0.1 if "embed" in name or "shared" in name else p.shape[-1] ** -0.5))

    def clip_ids(seed, V=512, B=2, L=77):
        ids = torch.randint(1, V - 2, (B, L), generator=torch.Generator().manual_seed(seed))
        for b in range(B):
            n = 6 + 40 * b
            ids[b, 0], ids[b, n], ids[b, n + 1:] = V - 2, V - 1, 0      # start of text, end of text (the highest id), padding
        return ids.cuda()

    def flat(out, prefix=""):
        """{name: tensor} of a tensor, a tuple or a dictionary of outputs (None entries dropped)"""
        if torch.is_tensor(out):
            return {prefix.rstrip(".") or "out": out}
        items = out.items() if isinstance(out, dict) else enumerate(out)
        return {k: v for key, val in items if val is not None for k, v in flat(val, f"{prefix}{key}.").items()}

    def frozen(case, tower, state, ids, **kwargs):
        tower.load_state_dict(state)
        tower = tower.cuda().requires_grad_(False)
        recorded(case, "FIRST", lambda: tower(ids, **kwargs))
        emit(case, **flat(recorded(case, "CALL", lambda: tower(ids, **kwargs))))

    def trained(case, module, forward, parameters, names, ids, seed):
        """two micro-batches of forward + backward under a FlatParamStore: overwrite, then accumulate"""
        module.cuda()
        store = FlatParamStore(parameters)
        g = torch.Generator().manual_seed(seed)
        cot = None
        for step, kind in enumerate(("FIRST", "CALL")):
            store.state.grad_accumulate = step == 1

            def run():
                nonlocal cot
                outs = flat(forward(ids))
                if cot is None:
                    cot = [torch.randn(o.shape, generator=g).cuda() for o in outs.values()]
                torch.autograd.backward(list(outs.values()), cot)
                return outs

            outs = recorded(case, kind, run)
            ids_of = {id(p) for p in parameters}
            grads = {f"grad{step}.{n}": p.grad for n, p in names.items() if id(p) in ids_of}
            assert all(gr is not None for gr in grads.values()), f"{case}: a trained parameter has no gradient"
            emit(case, **({f"out.{k}": v for k, v in outs.items()} if step == 0 else {}), **grads)
        store.state.grad_accumulate = False

    def state_of(tower, seed):
        randomize(tower, seed)
        return {k: v.detach().clone() for k, v in tower.state_dict().items()}

    for act in ("quick_gelu", "gelu"):
        cfg = dict(HF, hidden_act=act)
        state, ids = state_of(CLIPTextTower(**cfg), 10), clip_ids(11)
        frozen(f"hf-{act}-frozen", CLIPTextTower(**cfg), state, ids, output_hidden_states=True)
        selections = [("last", None), ("pooled", None), ("penultimate", None)] + [("hidden", i) for i in range(HF["num_hidden_layers"])]
        for layer, idx in selections:
            for pooled in (False, True):
                emb = FrozenCLIPEmbedder(device="cuda", config=cfg, layer=layer, layer_idx=idx, always_return_pooled=pooled, is_trainable=True)
                emb.transformer.load_state_dict(state)
                trained(f"hf-{act}-{layer}{'' if idx is None else idx}{'+pooled' if pooled else ''}", emb, emb, emb.trained_parameters(),
                        dict(emb.transformer.named_parameters()), ids, 12)

    state, ids = state_of(OpenCLIPTextTower(**OPEN_CLIP), 20), clip_ids(21)
    frozen("openclip-frozen", OpenCLIPTextTower(**OPEN_CLIP), state, ids)
    for layer in ("last", "pooled", "penultimate"):
        for pooled in (False, True):
            emb = FrozenOpenCLIPEmbedder2(device="cuda", config=OPEN_CLIP, layer=layer, always_return_pooled=pooled, is_trainable=True)
            emb.model.load_state_dict(state)
            trained(f"openclip-{layer}{'+pooled' if pooled else ''}", emb, emb, emb.trained_parameters(), dict(emb.model.named_parameters()), ids, 22)

    for proj in ("gated-gelu", "relu"):
        cfg = dict(T5, feed_forward_proj=proj)
        state = state_of(T5EncoderTower(**cfg), 30)
        for L in T5_LENGTHS:
            ids = torch.randint(0, T5["vocab_size"], (2, L), generator=torch.Generator().manual_seed(31 + L)).cuda()
            frozen(f"t5-{proj}-L{L}-frozen", T5EncoderTower(**cfg), state, ids)
            tower = T5EncoderTower(**cfg)
            tower.load_state_dict(state)
            trained(f"t5-{proj}-L{L}", tower, tower.train_outputs, list(tower.parameters()), dict(tower.named_parameters()), ids, 32)
    print("CHILD_DONE", flush=True)


def run_child(root: str, limit: int) -> list | None:
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--root", str(Path(root).resolve())], capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{root}: no result within {limit} s", file=sys.stderr)
        return None
    if r.returncode != 0 or "CHILD_DONE" not in r.stdout:
        print(f"{root}: exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr)
        return None
    return [line for line in r.stdout.splitlines() if line.split(" ")[0] in ("ROW", "CALL", "FIRST")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="(child) the source tree to import")
    ap.add_argument("--a", help="the parent commit's tree (built)")
    ap.add_argument("--b", help="this tree (built)")
    ap.add_argument("--label-a", default="the parent commit")
    ap.add_argument("--label-b", default="this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, args.root)
        child()
        return 0
    a = run_child(args.a, args.limit)
    if a is None:
        return 2      # the second child is not started
    b = run_child(args.b, args.limit)
    if b is None:
        return 2

    def by_case(lines, kind):
        cases = collections.OrderedDict()
        for line in lines:
            k, case, rest = line.split(" ", 2)
            if k == kind:
                cases.setdefault(case, []).append(rest)
        return cases

    digest = lambda rows: hashlib.sha256("\n".join(rows).encode()).hexdigest()[:16]
    text = [f"# Text towers, a = {args.label_a}, b = {args.label_b} (tools/ab_text_tower_bits.py).  Per case: the number of tensors (every output, every",
            "# trained parameter's gradient after an overwriting and after an accumulating micro-batch) and a digest of their sha256 list; the number of",
            "# steady-state launches (entry point + integer / float arguments, in order) and a digest of that list.",
            f"# {'case':<34} {'tensors':>7} {'a':<16} {'b':<10} {'launches':>8} {'a':<16} b"]
    rows_a, rows_b, calls_a, calls_b = by_case(a, "ROW"), by_case(b, "ROW"), by_case(a, "CALL"), by_case(b, "CALL")
    differ = []
    for case in rows_a:
        same_rows, same_calls = rows_a[case] == rows_b.get(case), calls_a.get(case) == calls_b.get(case)
        if not (same_rows and same_calls):
            differ.append(case)
        text.append(f"{case:<36} {len(rows_a[case]):>7} {digest(rows_a[case])} {'equal' if same_rows else 'DIFFERENT':<10} {len(calls_a.get(case, [])):>8} "
                    f"{digest(calls_a.get(case, []))} {'equal' if same_calls else 'DIFFERENT ' + digest(calls_b.get(case, []))}")
    n_rows, n_calls = sum(len(v) for v in rows_a.values()), sum(len(v) for v in calls_a.values())
    ok = not differ and list(rows_a) == list(rows_b)
    text.append(f"# {len(rows_a)} cases, {n_rows} tensors, {n_calls} steady-state launches: " + ("all equal" if ok else f"{len(differ)} cases DIFFER: " + ", ".join(differ[:20])))
    text.append("#\n# The first call of every case (it also builds the bf16 copies): launches per entry point where the trees differ, summed over the cases")
    first_a, first_b = by_case(a, "FIRST"), by_case(b, "FIRST")
    count = lambda first: collections.Counter(name for rows in first.values() for name in rows)
    ca, cb = count(first_a), count(first_b)
    for name in sorted(set(ca) | set(cb)):
        if ca[name] != cb[name]:
            text.append(f"#   {name:<28} a {ca[name]:>5}   b {cb[name]:>5}")
    text.append(f"#   every other entry point is launched equally often; the cases whose first call differs, of {len(first_a)}:")
    for case in first_a:
        da, db = collections.Counter(first_a[case]), collections.Counter(first_b.get(case, []))
        if da != db:
            text.append(f"#   {case:<34} " + ", ".join(f"{name} {da[name]} -> {db[name]}" for name in sorted(set(da) | set(db)) if da[name] != db[name]))
    out = "\n".join(text) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)
    print("\n".join(text[-8:]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
