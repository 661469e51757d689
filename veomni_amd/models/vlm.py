"""Qwen2.5-VL modeling (windowed vision tower + mrope language model),
written MI355X-first against the OpSlot API (no HF dependency).

Parity anchors (all in /root/reference/veomni/models/transformers/qwen2_5vl/
generated/patched_modeling_qwen2_5_vl_gpu.py):
  - patch embed :326-350 (Conv3d with stride == kernel, expressed here as
    the equivalent linear over flattened patches);
  - vision rotary :352-400 (h/w interleaved position ids, fp32 rope);
  - window index / cu_window_seqlens :161-244 (the host-side metadata port)
    — the same algorithm our PackingCollator already golden-matches;
  - vision attention :446-535 (qkv bias, NON-causal varlen over cu_seqlens;
    window blocks except config.fullatt_block_indexes, :831-846);
  - patch merger :366-380 (RMSNorm(1e-6) -> Linear -> GELU -> Linear);
  - 3D rope index :1368-1545 (get_vision_position_ids + get_rope_index);
  - feature insertion + language model :1660-1890 (masked_scatter at the
    image token id; mrope sections merged once per forward — see
    RotaryEmbedding in modeling.py).

MI355X design notes:
  - the vision tower's windowed attention runs as ONE SDPA call per block
    over a block-diagonal mask built from the (collator-precomputable)
    cu_seqlens — vision head_dim (80) is off the hand-written D=128 flash
    pair's path; the language model runs the standard HIP op stack
    (hip_flash attention incl. varlen, HIP rms/rope/swiglu/CE).
  - under Ulysses SP the vision tower is REPLICATED (every rank computes
    the full image set; deviation from the reference's ViT SP-slicing —
    simpler, correct, and the tower is a small fraction of step FLOPs);
    the text path stays SP-sliced, with the feature scatter done on the
    gathered sequence exactly like the reference (:1774-1840).
  - image modality only this round (the reference's video path mirrors the
    image path with temporal intervals; the data side already packs video
    keys).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..distributed.parallel_state import get_parallel_state
from .modeling import (ForCausalLM, ModelConfig, RMSNorm, rotate_half)


@dataclass
class VisionConfig:
    depth: int = 32
    hidden_size: int = 1280
    num_heads: int = 16
    intermediate_size: int = 3420
    out_hidden_size: int = 3584
    patch_size: int = 14
    temporal_patch_size: int = 2
    in_channels: int = 3
    spatial_merge_size: int = 2
    window_size: int = 112
    fullatt_block_indexes: tuple = (7, 15, 23, 31)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def merge_unit(self) -> int:
        return self.spatial_merge_size * self.spatial_merge_size


@dataclass
class VLConfig:
    text: ModelConfig = field(default_factory=ModelConfig)
    vision: VisionConfig = field(default_factory=VisionConfig)
    image_token_id: int = 151655
    name: str = "vl"


class VisionPatchEmbed(nn.Module):
    """Conv3d(stride == kernel) == one linear over the flattened patch
    (ref :326-350); the weight keeps the Conv3d shape so reference state
    dicts load with a reshape."""

    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.in_features = cfg.in_channels * cfg.temporal_patch_size * cfg.patch_size ** 2
        self.proj = nn.Linear(self.in_features, cfg.hidden_size, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(x.view(-1, self.in_features).to(self.proj.weight.dtype))


class VisionMLP(nn.Module):
    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.gate_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=True)
        self.up_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=True)
        self.down_proj = nn.Linear(cfg.intermediate_size, cfg.hidden_size, bias=True)

    def forward(self, x):
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


def _apply_vision_rope(q, k, cos, sin):
    """fp32 rope on [S, heads, D] (ref :389-400)."""
    qd, kd = q.dtype, k.dtype
    q, k = q.float(), k.float()
    cos = cos.unsqueeze(-2).float()
    sin = sin.unsqueeze(-2).float()
    q = (q * cos) + (rotate_half(q) * sin)
    k = (k * cos) + (rotate_half(k) * sin)
    return q.to(qd), k.to(kd)


class VisionAttention(nn.Module):
    """NON-causal varlen attention over [S, hidden] (ref :446-535):
    block-diagonal segments (full-attention blocks use the per-image
    cu_seqlens, window blocks the window cu_seqlens), executed as MASKLESS
    batched SDPA over runs of equal-length segments — numerically identical
    to the bool-masked single call, but it keeps torch on the flash/
    mem-efficient backend (a bool attn_mask forces the math path, which
    materializes [h, S, S] scores: 5+ GiB and an OOM at the seq-8192 mbs-4
    VLM bench shape)."""

    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.num_heads = cfg.num_heads
        self.head_dim = cfg.head_dim
        self.qkv = nn.Linear(cfg.hidden_size, cfg.hidden_size * 3, bias=True)
        self.proj = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.scaling = self.head_dim ** -0.5

    def forward(self, x, cu, cos, sin):
        S = x.shape[0]
        q, k, v = (self.qkv(x).reshape(S, 3, self.num_heads, -1)
                   .permute(1, 0, 2, 3).unbind(0))
        q, k = _apply_vision_rope(q, k, cos, sin)
        out = torch.empty_like(v)            # [S, h, D]
        i = 0
        n_seg = len(cu) - 1
        while i < n_seg:
            j = i
            L = cu[i + 1] - cu[i]
            while j < n_seg and cu[j + 1] - cu[j] == L:
                j += 1
            s0, s1, n = cu[i], cu[j], j - i
            qs = q[s0:s1].reshape(n, L, self.num_heads, -1).transpose(1, 2)
            ks = k[s0:s1].reshape(n, L, self.num_heads, -1).transpose(1, 2)
            vs = v[s0:s1].reshape(n, L, self.num_heads, -1).transpose(1, 2)
            o = F.scaled_dot_product_attention(qs, ks, vs, scale=self.scaling,
                                               is_causal=False)
            out[s0:s1] = o.transpose(1, 2).reshape(n * L, self.num_heads, -1)
            i = j
        return self.proj(out.reshape(S, -1))


class VisionBlock(nn.Module):
    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.norm1 = RMSNorm(cfg.hidden_size, eps=1e-6)
        self.norm2 = RMSNorm(cfg.hidden_size, eps=1e-6)
        self.attn = VisionAttention(cfg)
        self.mlp = VisionMLP(cfg)

    def forward(self, x, cu, cos, sin):
        x = x + self.attn(self.norm1(x), cu, cos, sin)
        x = x + self.mlp(self.norm2(x))
        return x


class PatchMerger(nn.Module):
    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.hidden_size = cfg.hidden_size * cfg.merge_unit
        self.ln_q = RMSNorm(cfg.hidden_size, eps=1e-6)
        self.mlp = nn.Sequential(
            nn.Linear(self.hidden_size, self.hidden_size),
            nn.GELU(),
            nn.Linear(self.hidden_size, cfg.out_hidden_size),
        )

    def forward(self, x):
        return self.mlp(self.ln_q(x).view(-1, self.hidden_size))


def vision_pos_ids(grid_list: List, merge: int) -> torch.Tensor:
    """Per-patch (h, w) position ids in the merge-interleaved patch order
    (ref :724-740): within each image, patches are laid out h-major but
    grouped into merge x merge cells."""
    parts = []
    for t, h, w in grid_list:
        hp = torch.arange(h).view(h, 1).expand(h, w)
        hp = hp.reshape(h // merge, merge, w // merge, merge).transpose(1, 2).flatten()
        wp = torch.arange(w).view(1, w).expand(h, w)
        wp = wp.reshape(h // merge, merge, w // merge, merge).transpose(1, 2).flatten()
        parts.append(torch.stack([hp, wp], dim=-1).repeat(t, 1))
    return torch.cat(parts, dim=0)


def vision_window_index(grid_list: List, cfg: VisionConfig):
    """Window permutation + cu_seqlens (full + window) for the packed image
    set — same contract as the reference's get_window_index / the collator's
    vit metadata port (:161-244). Returns (window_index [n_units],
    cu_seqlens list, cu_window list)."""
    merge = cfg.spatial_merge_size
    unit = cfg.merge_unit
    wpm = cfg.window_size // merge // cfg.patch_size   # merged cells / window

    cu = [0]
    for t, h, w in grid_list:
        for _ in range(t):
            cu.append(cu[-1] + h * w)

    parts, cu_win, base = [], [0], 0
    for t, h, w in grid_list:
        gh, gw = h // merge, w // merge
        idx = torch.arange(t * gh * gw).reshape(t, gh, gw)
        ph, pw = (-gh) % wpm, (-gw) % wpm
        nh, nw = (gh + ph) // wpm, (gw + pw) // wpm
        padded = F.pad(idx, (0, pw, 0, ph), value=-100)
        padded = padded.reshape(t, nh, wpm, nw, wpm).permute(0, 1, 3, 2, 4)
        padded = padded.reshape(t, nh * nw, wpm, wpm)
        lens = (padded != -100).sum(dim=(2, 3)).reshape(-1)
        flat = padded.reshape(-1)
        parts.append(flat[flat != -100] + base)
        for n in (lens.cumsum(0) * unit + cu_win[-1]).tolist():
            if n != cu_win[-1]:
                cu_win.append(n)
        base += t * gh * gw
    return torch.cat(parts), cu, cu_win


class VisionTower(nn.Module):
    """Windowed ViT (ref :616-905). Forward takes the packed patch tensor
    and the host-side grid list; returns merged features [n_units, out_h]."""

    def __init__(self, cfg: VisionConfig):
        super().__init__()
        self.cfg = cfg
        self.patch_embed = VisionPatchEmbed(cfg)
        inv = 1.0 / (10000.0 ** (torch.arange(0, cfg.head_dim // 2, 2, dtype=torch.float32)
                                 / (cfg.head_dim // 2)))
        self.register_buffer("rot_inv_freq", inv, persistent=False)
        self.blocks = nn.ModuleList(VisionBlock(cfg) for _ in range(cfg.depth))
        self.merger = PatchMerger(cfg)

    def forward(self, pixel_values: torch.Tensor, grid_list: List) -> torch.Tensor:
        cfg = self.cfg
        x = self.patch_embed(pixel_values)
        S = x.shape[0]

        pos = vision_pos_ids(grid_list, cfg.spatial_merge_size).to(x.device)
        freqs = (pos.unsqueeze(-1).float() * self.rot_inv_freq).flatten(1)  # [S, hd/4*2]
        window_index, cu, cu_win = vision_window_index(grid_list, cfg)
        window_index = window_index.to(x.device)

        # permute into window order at merge-unit granularity (ref :788-796)
        unit = cfg.merge_unit
        x = x.reshape(S // unit, unit, -1)[window_index].reshape(S, -1)
        freqs = freqs.reshape(S // unit, unit, -1)[window_index].reshape(S, -1)
        emb = torch.cat((freqs, freqs), dim=-1)
        cos, sin = emb.cos(), emb.sin()

        for i, blk in enumerate(self.blocks):
            seg = cu if i in cfg.fullatt_block_indexes else cu_win
            x = blk(x, seg, cos, sin)

        merged = self.merger(x)                      # [S/unit, out_hidden]
        reverse = torch.argsort(window_index)
        return merged[reverse]


def vl_position_ids(input_ids: torch.Tensor, image_token_id: int,
                    grid_list: List, merge: int) -> torch.Tensor:
    """3D (t, h, w) rope index for an image+text sequence
    (ref get_rope_index :1426-1543 + get_vision_position_ids :1368-1424).
    Text runs advance all three axes together; each image run contributes a
    (1, gh, gw) grid offset by the running position; after an image the
    position advances by max(gh, gw)."""
    B, S = input_ids.shape
    out = torch.zeros(3, B, S, dtype=torch.long)
    grids = iter(grid_list)
    for b in range(B):
        ids = input_ids[b].tolist()
        pos_list = []
        cur = 0
        i = 0
        while i < S:
            is_img = ids[i] == image_token_id
            j = i
            while j < S and (ids[j] == image_token_id) == is_img:
                j += 1
            n = j - i
            if not is_img:
                seg = torch.arange(n).view(1, -1).expand(3, -1) + cur
                pos_list.append(seg)
                cur += n
            else:
                t, h, w = next(grids)
                gt, gh, gw = t, h // merge, w // merge
                assert gt * gh * gw == n, (t, h, w, n)
                pt = torch.arange(gt).repeat_interleave(gh * gw) + cur
                ph = torch.arange(gh).repeat_interleave(gw).repeat(gt) + cur
                pw = torch.arange(gw).repeat(gh * gt) + cur
                pos_list.append(torch.stack([pt, ph, pw]))
                cur += max(gh, gw)
            i = j
        out[:, b] = torch.cat(pos_list, dim=1)
    return out


class VLForCausalLM(ForCausalLM):
    """Qwen2.5-VL: vision tower + the standard decoder with mrope.
    Reuses ForCausalLM's loss path (fused chunked CE) and decoder stack
    (HIP attention incl. varlen, rms/rope/swiglu kernels)."""

    def __init__(self, config: VLConfig):
        super().__init__(config.text)
        self.vl_config = config
        self.visual = VisionTower(config.vision)
        self.reset_parameters()

    def forward(self, input_ids, labels=None, position_ids=None,
                pixel_values=None, image_grid_thw=None, **kwargs):
        cfg = self.vl_config
        ps = get_parallel_state()
        embeds = self.model.embed_tokens(input_ids)

        if pixel_values is not None:
            if image_grid_thw is None:
                raise ValueError("pixel_values without image_grid_thw")
            grid_list = (image_grid_thw.tolist()
                         if torch.is_tensor(image_grid_thw) else list(image_grid_thw))
            feats = self.visual(pixel_values, grid_list).to(embeds.dtype)
            if ps.sp_enabled:
                # scatter on the gathered sequence, then re-slice
                # (ref Patch.1/Patch.2 :1774-1830; the tower itself is
                # replicated — see module docstring)
                from ..distributed.sequence_parallel import (
                    gather_outputs, slice_input_tensor)
                import torch.distributed as dist

                ids_g = [torch.zeros_like(input_ids) for _ in range(ps.sp_size)]
                dist.all_gather(ids_g, input_ids, group=ps.sp_group)
                ids_full = torch.cat(ids_g, dim=1)
                embeds = gather_outputs(embeds, gather_dim=1, group=ps.sp_group)
                mask = (ids_full == cfg.image_token_id)
                embeds = embeds.masked_scatter(
                    mask.unsqueeze(-1).expand_as(embeds), feats)
                embeds = slice_input_tensor(embeds, dim=1, group=ps.sp_group)
                if position_ids is None:
                    pos3 = vl_position_ids(ids_full.cpu(), cfg.image_token_id,
                                           grid_list, cfg.vision.spatial_merge_size)
                    sl = ids_full.shape[1] // ps.sp_size
                    r = ps.sp_rank
                    position_ids = pos3[:, :, r * sl:(r + 1) * sl].to(input_ids.device)
            else:
                mask = (input_ids == cfg.image_token_id)
                embeds = embeds.masked_scatter(
                    mask.unsqueeze(-1).expand_as(embeds), feats)
                if position_ids is None:
                    position_ids = vl_position_ids(
                        input_ids.cpu(), cfg.image_token_id, grid_list,
                        cfg.vision.spatial_merge_size).to(input_ids.device)

        return super().forward(input_ids, labels=labels,
                               position_ids=position_ids,
                               inputs_embeds=embeds, **kwargs)

    @torch.no_grad()
    def reset_parameters(self, seed: int = 1234):
        if not hasattr(self, "visual"):
            return  # called from ForCausalLM.__init__ before visual exists
        std = self.config.initializer_range
        try:
            dev = next(self.parameters()).device
        except StopIteration:
            return
        if dev.type == "meta":
            return
        g = torch.Generator(device=dev).manual_seed(seed)
        for name, p in sorted(self.named_parameters(), key=lambda kv: kv[0]):
            if (name.endswith("layernorm.weight") or name.endswith("norm.weight")
                    or ".q_norm" in name or ".k_norm" in name
                    or name.endswith("norm1.weight") or name.endswith("norm2.weight")
                    or name.endswith("ln_q.weight")):
                p.fill_(1.0)
            elif name.endswith(".bias") or name.endswith("_bias"):
                p.zero_()
            else:
                buf = torch.empty(p.shape, dtype=torch.float32, device=dev)
                buf.normal_(0.0, std, generator=g)
                p.copy_(buf.to(p.dtype))
