"""Checkpoint loading: safetensors directory -> Qwen3Model, TP-shard aware.

The offline build environment has no checkpoint sources, so engines default to
deterministic random init — but the loading path is real: point
`EngineConfig.weights_path` (or engine_kwargs["weights_path"]) at a directory
of .safetensors files and each parameter is filled from its tensor, sliced per
the parameter's TP shard metadata (see `qwen3._mark_shard`).

Accepted checkpoint names: this framework's own `named_parameters()` names,
plus the conventional HF-style aliases (model.layers.N..., model.embed_tokens,
lm_head) mapped onto them. Merged projections (qkv_proj, gate_up_proj) also
accept split q/k/v and gate/up tensors.

MXFP4 experts (`moe_weight_dtype="mxfp4"`): `save_weights` writes quantised
experts as the uint8 pair `<...>.mlp.gate_up_blocks` / `.gate_up_scales` and
`.down_blocks` / `.down_scales` (the format of
`torch_ref.quantize_weight_mxfp4`), and `load_weights(...,
moe_weight_dtype="mxfp4")` copies such a pair into the model bit for bit,
without a bf16 stage. The pair must have the shape of the local shard (it is
not re-sliced for TP/EP). The published gpt-oss tensor names are not mapped.

Block-FP8 dense projections (`dense_weight_dtype="fp8_block128"`): the layout
of the published Qwen3 `-FP8` checkpoints. A projection (qkv / o / gate_up /
down, under the merged or the split q/k/v and gate/up names) may come as
`<proj>.weight` of dtype float8_e4m3fn [N, K] together with
`<proj>.weight_scale_inv` f32 [N/128, K/128], one scale per 128x128 block.
`load_weights(..., dense_weight_dtype="fp8_block128")` copies the pair into
the model bit for bit, without a bf16 stage: split tensors are merged by
concatenating codes along N and scales along dim 0 (each part needs
N % 128 == 0), and TP shards cut codes and scales together (column-parallel
projections along N/128, row-parallel ones along K/128; a shard boundary
that is not a multiple of 128 is an error). Projections that come as bf16 are
loaded as always and left for the engine to quantise. With any other
`dense_weight_dtype` an e4m3 `weight` is an error, never an upcast of the
bare codes. A `config.json` beside the files that carries a
`quantization_config` must say `quant_method: "fp8"` with
`weight_block_size: [128, 128]`. `save_weights` writes a block-quantised
model under its own merged names, so the file reloads the same way. The
model is still built in bf16 before such a load, so peak memory at load is
the bf16 model's.

Attention sinks (`EngineConfig.local_attention` with a spec that has them):
the parameter is `layers.N.self_attn.sinks`, f32 [num_heads], the name gpt-oss
checkpoints use (`model.layers.N.self_attn.sinks`); it is sliced with the q
heads under TP and is required under strict=True. A model built without sinks
has no such parameter, so a checkpoint that carries them reports the tensors
as unexpected (strict=True) or skips them (strict=False), like any other.
"""

from __future__ import annotations

import json
import os
import re
from typing import Dict, Iterator, List, Tuple

import torch

# pre-quantised MXFP4 experts: ...mlp.<gate_up|down>_<blocks|scales>
_MXFP4_RE = re.compile(r"^(.*\.mlp)\.(gate_up|down)_(blocks|scales)$")

# HF per-expert tensors: ...mlp.experts.<E>.<gate|up|down>_proj.weight
_EXPERT_RE = re.compile(r"^(.*\.mlp)\.experts\.(\d+)\.(gate|up|down)_proj\.weight$")


def _iter_safetensors(path: str) -> Iterator[Tuple[str, torch.Tensor]]:
    from safetensors import safe_open

    files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if not files:
        raise FileNotFoundError(f"no .safetensors files under {path!r}")
    for fn in files:
        with safe_open(os.path.join(path, fn), framework="pt") as f:
            for name in f.keys():
                yield name, f.get_tensor(name)


def _canon(name: str) -> str:
    """HF-style name -> this model's name."""
    n = name
    if n.startswith("model."):
        n = n[len("model."):]
    return n


def _shard_slice(p: torch.nn.Parameter, full: torch.Tensor) -> torch.Tensor:
    """Apply the parameter's TP shard metadata to a full checkpoint tensor."""
    tp_size = getattr(p, "_tp_size", 1)
    if tp_size <= 1 or tuple(full.shape) == tuple(p.shape):
        return full
    dim, rank = p._tp_dim, p._tp_rank
    sections = p._tp_sections or [(0, full.shape[dim])]
    parts = []
    for start, length in sections:
        per = length // tp_size
        parts.append(full.narrow(dim, start + rank * per, per))
    return torch.cat(parts, dim=dim)


_FP8_SCALE_SUFFIX = ".weight_scale_inv"


def _check_quantization_config(path: str) -> None:
    """A config.json with a quantization_config must describe the one
    pre-quantised dense format the loader reads."""
    cfg_path = os.path.join(path, "config.json")
    if not os.path.isfile(cfg_path):
        return
    with open(cfg_path) as f:
        qc = json.load(f).get("quantization_config")
    if qc is None:
        return
    block = qc.get("weight_block_size")
    if (qc.get("quant_method") != "fp8" or block is None
            or list(block) != [128, 128]):
        raise ValueError(
            f"{cfg_path}: unsupported quantization_config (quant_method="
            f"{qc.get('quant_method')!r}, weight_block_size={block!r}); only "
            "quant_method 'fp8' with weight_block_size [128, 128] loads")


def _shard_slice_fp8_block(p: torch.nn.Parameter, name: str,
                           codes: torch.Tensor, scales: torch.Tensor):
    """`_shard_slice` for a block-quantised pair: codes [N, K] and scales
    [N/128, K/128] are cut together, so every cut must fall on a block."""
    tp_size = getattr(p, "_tp_size", 1)
    if tp_size <= 1 or tuple(codes.shape) == tuple(p.shape):
        return codes, scales
    dim, rank = p._tp_dim, p._tp_rank
    sections = p._tp_sections or [(0, codes.shape[dim])]
    c_parts, s_parts = [], []
    for start, length in sections:
        per = length // tp_size
        lo = start + rank * per
        if lo % 128 or per % 128:
            raise ValueError(
                f"{name}: TP shard [{lo}, {lo + per}) along dim {dim} does "
                "not fall on the 128-wide scale blocks")
        c_parts.append(codes.narrow(dim, lo, per))
        s_parts.append(scales.narrow(dim, lo // 128, per // 128))
    return torch.cat(c_parts, dim=dim), torch.cat(s_parts, dim=dim)


def load_weights(model: torch.nn.Module, path: str, strict: bool = True,
                 moe_weight_dtype: str = "bf16",
                 dense_weight_dtype: str = "bf16") -> int:
    """Fill `model` from a safetensors dir. Returns #parameters loaded.
    With moe_weight_dtype="mxfp4" a checkpoint may hold experts as the
    quantised uint8 pair (see the module docstring); bf16 experts are loaded
    as always and left for the engine to quantise. With
    dense_weight_dtype="fp8_block128" it may hold dense projections as the
    e4m3 `weight` + f32 `weight_scale_inv` pair (module docstring); with any
    other value such a tensor is a ValueError."""
    _check_quantization_config(path)
    params: Dict[str, torch.nn.Parameter] = dict(model.named_parameters())
    modules = dict(model.named_modules())
    # block-FP8 dense pairs: target parameter -> part -> {"weight", "scale"}
    pending_fp8: Dict[str, Dict[str, Dict[str, torch.Tensor]]] = {}
    pending_mxfp4: Dict[Tuple[str, str], Dict[str, torch.Tensor]] = {}
    pending_merge: Dict[str, Dict[str, torch.Tensor]] = {}
    loaded = set()

    def assign(pname: str, tensor: torch.Tensor) -> None:
        p = params[pname]
        t = _shard_slice(p, tensor)
        if tuple(t.shape) != tuple(p.shape):
            raise ValueError(
                f"shape mismatch for {pname}: checkpoint {tuple(tensor.shape)} "
                f"-> shard {tuple(t.shape)} vs parameter {tuple(p.shape)}")
        with torch.no_grad():
            p.copy_(t.to(p.dtype))
        loaded.add(pname)

    merge_map = {
        "q_proj.weight": ("qkv_proj.weight", "q"),
        "k_proj.weight": ("qkv_proj.weight", "k"),
        "v_proj.weight": ("qkv_proj.weight", "v"),
        "gate_proj.weight": ("gate_up_proj.weight", "gate"),
        "up_proj.weight": ("gate_up_proj.weight", "up"),
    }

    def dense_target(wname: str):
        """`<proj>.weight` (merged or split name) -> (parameter name, part)
        when it names a dense projection of this model, else None."""
        if wname in params and isinstance(
                modules.get(wname[: -len(".weight")]), torch.nn.Linear):
            return wname, "all"
        for suffix, (target_suffix, part) in merge_map.items():
            if wname.endswith(suffix):
                target = wname[: -len(suffix)] + target_suffix
                if target in params:
                    return target, part
        return None

    pending_experts: Dict[str, Dict[Tuple[int, str], torch.Tensor]] = {}
    unexpected: List[str] = []
    for raw_name, tensor in _iter_safetensors(path):
        name = _canon(raw_name)
        is_scale = name.endswith(_FP8_SCALE_SUFFIX)
        if is_scale or tensor.dtype == torch.float8_e4m3fn:
            wname = name[: -len("_scale_inv")] if is_scale else name
            hit = dense_target(wname) if wname.endswith(".weight") else None
            if hit is None and is_scale:
                unexpected.append(raw_name)
                continue
            if hit is None or dense_weight_dtype != "fp8_block128":
                # never upcast bare codes, whatever `strict` says
                raise ValueError(
                    f"checkpoint holds FP8 tensor {raw_name}; only dense "
                    "projections load as e4m3, with dense_weight_dtype="
                    f"'fp8_block128' (got {dense_weight_dtype!r})")
            pending_fp8.setdefault(hit[0], {}).setdefault(hit[1], {})[
                "scale" if is_scale else "weight"] = tensor
            continue
        if name in params:
            assign(name, tensor)
            continue
        mm = _MXFP4_RE.match(name)
        if mm and f"{mm.group(1)}.{mm.group(2)}" in params:
            if moe_weight_dtype != "mxfp4":
                raise ValueError(
                    f"checkpoint holds MXFP4 experts ({raw_name}); load it "
                    f"with moe_weight_dtype='mxfp4', not {moe_weight_dtype!r}")
            pending_mxfp4.setdefault((mm.group(1), mm.group(2)), {})[
                mm.group(3)] = tensor
            continue
        em = _EXPERT_RE.match(name)
        if em and f"{em.group(1)}.gate_up" in params:
            # per-expert stacked MoE weights ([E, N, K] layout = per-expert
            # torch-Linear tensors stacked, so copies are direct)
            pending_experts.setdefault(em.group(1), {})[
                (int(em.group(2)), em.group(3))] = tensor
            continue
        # split projections to be merged
        for suffix, (target_suffix, part) in merge_map.items():
            if name.endswith(suffix):
                prefix = name[: -len(suffix)]
                target = prefix + target_suffix
                if target in params:
                    pending_merge.setdefault(target, {})[part] = tensor
                    break
        else:
            if name == "lm_head.weight" and "lm_head.weight" not in params:
                continue  # tied embeddings
            unexpected.append(raw_name)

    for target, parts in pending_merge.items():
        if target.endswith("qkv_proj.weight"):
            needed = ("q", "k", "v")
        else:
            needed = ("gate", "up")
        if not all(k in parts for k in needed):
            raise ValueError(f"incomplete split tensors for {target}: "
                             f"{sorted(parts)}")
        assign(target, torch.cat([parts[k] for k in needed], dim=0))

    for target, parts in pending_fp8.items():
        if target.endswith("qkv_proj.weight") and "all" not in parts:
            needed = ("q", "k", "v")
        elif target.endswith("gate_up_proj.weight") and "all" not in parts:
            needed = ("gate", "up")
        else:
            needed = ("all",)
        if sorted(parts) != sorted(needed) or target in loaded:
            raise ValueError(f"incomplete or mixed FP8 tensors for {target}: "
                             f"{sorted(parts)}")
        for part in needed:
            pair = parts[part]
            if sorted(pair) != ["scale", "weight"]:
                raise ValueError(
                    f"incomplete FP8 pair for {target} ({part}): needs both "
                    f"weight and weight_scale_inv, has {sorted(pair)}")
            wq, sc = pair["weight"], pair["scale"]
            if (wq.dim() != 2 or wq.shape[0] % 128 or wq.shape[1] % 128
                    or sc.dtype != torch.float32
                    or tuple(sc.shape) != (wq.shape[0] // 128,
                                           wq.shape[1] // 128)):
                raise ValueError(
                    f"bad FP8 pair for {target} ({part}): weight "
                    f"{tuple(wq.shape)} needs N % 128 == 0, K % 128 == 0 and "
                    f"a float32 weight_scale_inv [N/128, K/128], got "
                    f"{sc.dtype} {tuple(sc.shape)}")
        codes = torch.cat([parts[k]["weight"] for k in needed], dim=0)
        scales = torch.cat([parts[k]["scale"] for k in needed], dim=0)
        p = params[target]
        codes, scales = _shard_slice_fp8_block(p, target, codes, scales)
        if tuple(codes.shape) != tuple(p.shape):
            raise ValueError(
                f"shape mismatch for {target}: checkpoint shard "
                f"{tuple(codes.shape)} vs parameter {tuple(p.shape)}")
        from .qwen3 import install_linear_fp8_block128

        install_linear_fp8_block128(modules[target[: -len(".weight")]],
                                    codes, scales)
        loaded.add(target)

    for prefix, parts in pending_experts.items():
        n_exp = max(e for e, _ in parts) + 1
        for what, pname in (("gate/up", f"{prefix}.gate_up"),
                            ("down", f"{prefix}.down")):
            need = (("gate", "up") if what == "gate/up" else ("down",))
            full_e = []
            for e in range(n_exp):
                try:
                    full_e.append(torch.cat([parts[(e, k)] for k in need],
                                            dim=0))
                except KeyError:
                    raise ValueError(
                        f"incomplete expert tensors for {prefix} expert {e}")
            assign(pname, torch.stack(full_e))

    for (prefix, which), pair in pending_mxfp4.items():
        if sorted(pair) != ["blocks", "scales"]:
            raise ValueError(f"incomplete MXFP4 pair for {prefix}.{which}: "
                             f"{sorted(pair)}")
        modules[prefix].load_expert_mxfp4(which, pair["blocks"],
                                          pair["scales"])
        loaded.add(f"{prefix}.{which}")

    if unexpected and strict:
        raise ValueError(
            f"checkpoint has {len(unexpected)} tensors that map to no "
            f"parameter (strict=True): {unexpected[:6]}"
            f"{'...' if len(unexpected) > 6 else ''}")
    missing = [n for n, p in params.items()
               if n not in loaded and (p.dim() >= 2 or n.endswith(".sinks"))]
    if missing and strict:
        raise ValueError(f"checkpoint missing parameters: {missing[:8]}"
                         f"{'...' if len(missing) > 8 else ''}")
    return len(loaded)


def save_weights(model: torch.nn.Module, path: str) -> str:
    """Save the model's parameters as one safetensors file (testing/export)."""
    from safetensors.torch import save_file

    block_fp8 = {}
    for prefix, mod in model.named_modules():
        if (isinstance(mod, torch.nn.Linear)
                and mod.weight.dtype == torch.float8_e4m3fn):
            if getattr(mod, "weight_scale_inv", None) is not None:
                # block-quantised pair, under the published names
                block_fp8[f"{prefix}.weight"] = mod.weight
                block_fp8[f"{prefix}.weight_scale_inv"] = mod.weight_scale_inv
                continue
            # per-channel quantised projections are buffers, not parameters:
            # the file would silently lack them, and no loader reads them back
            raise RuntimeError(
                f"{prefix}.weight is stored as fp8_e4m3 "
                "(dense_weight_dtype): save the unquantised model; "
                "checkpoints of FP8 dense weights are not supported")
    os.makedirs(path, exist_ok=True)
    out = os.path.join(path, "model.safetensors")
    state = {k: v.detach().cpu().contiguous()
             for k, v in model.named_parameters()}
    state.update({k: v.detach().cpu().contiguous()
                  for k, v in block_fp8.items()})
    for prefix, mod in model.named_modules():
        if getattr(mod, "experts_mxfp4", False):
            for which in ("gate_up", "down"):
                state[f"{prefix}.{which}_blocks"] = (
                    getattr(mod, which).detach().cpu().contiguous())
                state[f"{prefix}.{which}_scales"] = (
                    getattr(mod, which + "_scales").detach().cpu().contiguous())
    save_file(state, out)
    return out
