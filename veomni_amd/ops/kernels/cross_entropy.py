"""HIP chunked fused-linear cross-entropy (impl name "hip").

Parity targets:
  - ForCausalLMLoss 3-tuple contract + SP handling:
    ops/kernels/cross_entropy/__init__.py:89-221;
  - chunked fused-linear semantics (never materializes [T,V]):
    chunk_loss.py:43-144 — grads computed IN forward per chunk, saved,
    scaled by upstream grad in backward;
  - inner CE = fixed_cross_entropy: fp32 log-softmax, sum-NLL / num_items;
  - return_log_probs=True: per-token log p(y_t) and softmax entropy
    (chunk_logprobs.py), returned as FusedLinearAuxOutput in the third slot;
  - top-k forward-KL distillation against teacher_topk_ids /
    teacher_topk_log_probs (chunk_topk_distill.py), reached through
    hip_chunk_topk_distill_function and ForCausalLM.forward.

Device split: chunk logits/dW/dx GEMMs ride hipBLASLt via torch.matmul
(plain library GEMMs); the softmax/NLL/grad fusion is vh_ce_fwd, the
log-prob/entropy row pass and its gradient are vh_logprob_fwd/_bwd, the
top-k gather/KL row pass and the fused gradient are vh_topk_kl_fwd /
vh_topk_distill_bwd (C ABI).
"""

from __future__ import annotations

import torch

from ...distributed.parallel_state import get_parallel_state
from ...distributed.sequence_parallel import reduce_sequence_parallel_loss
from ...model_outputs import FusedLinearAuxOutput
from .. import hip_lib
from ..kernel_registry import KERNEL_REGISTRY, HardwareRequirement, KernelSpec

IGNORE_INDEX = -100
# stash-vs-stream switch for the dlogits buffer (test-patchable)
STASH_LIMIT_BYTES = 16 << 30


class HipChunkCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden_states, weight, labels, chunk_size):
        # hidden [B, T, H] (already causally aligned by the caller), labels [B, T]
        B, T, H = hidden_states.shape
        flat_h = hidden_states.reshape(-1, H)
        flat_l = labels.reshape(-1)
        num_items = (flat_l != IGNORE_INDEX).sum()
        inv = 1.0 / max(int(num_items), 1)

        total = torch.zeros((), dtype=torch.float32, device=hidden_states.device)
        # Fast path: stash per-chunk dlogits (bf16, [T, V]) so dgrad/wgrad run
        # as single full-T GEMMs with hipBLASLt's internal fp32 accumulation;
        # a per-chunk fp32 `grad_w +=` RMW measured ~1 ms/chunk of pure
        # elementwise traffic on the 8B vocab grad. Above 16 GiB of stash
        # (seq-16384 dynamic batches, config 5) switch to the reference
        # chunk_loss's no-[T,V] property: per-chunk dgrad/wgrad with an fp32
        # grad_w accumulator, peak extra memory = one [chunk, V] dlogits +
        # the fp32 [V, H] accumulator.
        T_flat, V = flat_h.shape[0], weight.shape[0]
        lowmem = T_flat * V * flat_h.element_size() > STASH_LIMIT_BYTES
        if lowmem:
            grad_h = torch.empty_like(flat_h)
            grad_w32 = torch.zeros(weight.shape, dtype=torch.float32,
                                   device=weight.device)
            for s in range(0, T_flat, chunk_size):
                e = min(s + chunk_size, T_flat)
                h = flat_h[s:e]
                logits = torch.matmul(h, weight.t())
                loss_rows, dlog = hip_lib.ce_fwd(logits, flat_l[s:e], inv,
                                                 IGNORE_INDEX)
                total += loss_rows.sum() * inv
                torch.matmul(dlog, weight, out=grad_h[s:e])
                grad_w32 += torch.matmul(dlog.t(), h).float()
            grad_w = grad_w32.to(weight.dtype)
        else:
            dlog_all = flat_h.new_empty((T_flat, V))
            for s in range(0, T_flat, chunk_size):
                e = min(s + chunk_size, T_flat)
                h = flat_h[s:e]
                logits = torch.matmul(h, weight.t())      # bf16 (hipBLASLt)
                loss_rows, _ = hip_lib.ce_fwd(logits, flat_l[s:e], inv,
                                              IGNORE_INDEX,
                                              dlogits_out=dlog_all[s:e])
                total += loss_rows.sum() * inv
            grad_h = torch.matmul(dlog_all, weight)
            grad_w = torch.matmul(dlog_all.t(), flat_h)
        ctx.save_for_backward(grad_h, grad_w)
        ctx.hshape = hidden_states.shape
        return total

    @staticmethod
    def backward(ctx, grad_output):
        grad_h, grad_w = ctx.saved_tensors
        if grad_output is not None and not torch.equal(
            grad_output, torch.ones_like(grad_output)
        ):
            grad_h = grad_h * grad_output
            grad_w = grad_w * grad_output
        return grad_h.reshape(ctx.hshape), grad_w, None, None


# --------------------------------------------------------------------------
# Per-token log-probs + entropy (the return_log_probs half of the contract)
# --------------------------------------------------------------------------
def _hip_logprobs_chunks(flat_h, weight, flat_l, temperature, chunk_size,
                         ignore_index, want_stats):
    """Chunked lm_head GEMM (bf16, hipBLASLt) + vh_logprob_fwd per chunk.
    Returns fp32 [T] (log_probs, entropy, lse|None, ent_raw|None)."""
    if flat_h.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise TypeError(
            "the hip log-probs path takes bf16 hidden_states and weights, got "
            f"{flat_h.dtype} / {weight.dtype}; bind the slot 'eager' for other dtypes")
    T_flat = flat_h.shape[0]
    parts = []
    for s in range(0, T_flat, chunk_size):
        e = min(s + chunk_size, T_flat)
        logits = torch.matmul(flat_h[s:e], weight.t())
        parts.append(hip_lib.logprob_fwd(logits, flat_l[s:e], temperature,
                                         ignore_index, want_stats=want_stats))
    if not parts:
        z = torch.zeros(0, dtype=torch.float32, device=flat_h.device)
        return z, z.clone(), (z.clone() if want_stats else None), \
            (z.clone() if want_stats else None)
    cols = [torch.cat(c) if c[0] is not None else None for c in zip(*parts)]
    return tuple(cols)


def _flat_labels(labels):
    return labels.reshape(-1).to(torch.int64).contiguous()


class HipChunkLogProbs(torch.autograd.Function):
    """(log_probs, entropy) through the lm_head without building [T, V].

    Forward keeps hidden/weight/labels plus the two fp32 [T] row statistics
    (lse, unmasked entropy); backward re-issues each chunk's logits GEMM
    exactly as forward did, so vh_logprob_bwd sees the same bf16 logits."""

    @staticmethod
    def forward(ctx, hidden_states, weight, labels, temperature, chunk_size,
                ignore_index):
        ctx.set_materialize_grads(False)
        flat_h = hidden_states.reshape(-1, hidden_states.shape[-1])
        flat_l = _flat_labels(labels)
        lp, ent, lse, raw = _hip_logprobs_chunks(
            flat_h, weight, flat_l, temperature, chunk_size, ignore_index,
            want_stats=True)
        ctx.save_for_backward(flat_h, weight, flat_l, lse, raw)
        ctx.temperature = temperature
        ctx.chunk_size = chunk_size
        ctx.ignore_index = ignore_index
        ctx.hshape = hidden_states.shape
        return lp.view(labels.shape), ent.view(labels.shape)

    @staticmethod
    def backward(ctx, dlog_probs, dentropy):
        if dlog_probs is None and dentropy is None:
            return None, None, None, None, None, None
        flat_h, weight, flat_l, lse, raw = ctx.saved_tensors
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_h or need_w):
            return None, None, None, None, None, None
        dlp = (dlog_probs.reshape(-1).float().contiguous()
               if dlog_probs is not None else None)
        dent = (dentropy.reshape(-1).float().contiguous()
                if dentropy is not None else None)
        T_flat, V = flat_h.shape[0], weight.shape[0]
        cs = ctx.chunk_size
        grad_h = torch.empty_like(flat_h) if need_h else None
        grad_w32 = (torch.zeros(weight.shape, dtype=torch.float32,
                                device=weight.device) if need_w else None)
        dlog_buf = flat_h.new_empty((min(cs, T_flat), V))
        for s in range(0, T_flat, cs):
            e = min(s + cs, T_flat)
            h = flat_h[s:e]
            logits = torch.matmul(h, weight.t())
            dlog = hip_lib.logprob_bwd(
                logits, flat_l[s:e], lse[s:e], raw[s:e],
                dlp[s:e] if dlp is not None else None,
                dent[s:e] if dent is not None else None,
                ctx.temperature, ctx.ignore_index, dlogits_out=dlog_buf[:e - s])
            if need_h:
                torch.matmul(dlog, weight, out=grad_h[s:e])
            if need_w:
                grad_w32 += torch.matmul(dlog.t(), h).float()
        grad_w = grad_w32.to(weight.dtype) if need_w else None
        if need_h:
            grad_h = grad_h.reshape(ctx.hshape)
        return grad_h, grad_w, None, None, None, None


class EagerChunkLogProbs(torch.autograd.Function):
    """Torch-only twin of HipChunkLogProbs; restates the reference's
    chunk_logprobs op for op (ref chunk_logprobs.py:165-189, :214-273), any
    dtype, any device: the temperature divides the logits in the input dtype
    before the fp32 upcast, dlogits is cast to the input dtype before it is
    divided, and dweight accumulates across chunks in the weight's dtype."""

    @staticmethod
    def _chunk_logits(h, weight, temperature):
        logits = h @ weight.t()
        if temperature != 1.0:
            logits = logits / temperature
        return logits.float()

    @staticmethod
    def forward(ctx, hidden_states, weight, labels, temperature, chunk_size,
                ignore_index):
        ctx.set_materialize_grads(False)
        flat_h = hidden_states.reshape(-1, hidden_states.shape[-1])
        flat_l = _flat_labels(labels)
        T_flat = flat_h.shape[0]
        lp = torch.zeros(T_flat, dtype=torch.float32, device=flat_h.device)
        ent = torch.zeros_like(lp)
        for s in range(0, T_flat, chunk_size):
            e = min(s + chunk_size, T_flat)
            logits = EagerChunkLogProbs._chunk_logits(flat_h[s:e], weight,
                                                      temperature)
            lab = flat_l[s:e]
            valid = lab != ignore_index
            at_label = logits.log_softmax(dim=-1).gather(
                -1, lab.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            probs = logits.softmax(dim=-1)
            H = torch.logsumexp(logits, dim=-1) - torch.sum(probs * logits, dim=-1)
            lp[s:e] = torch.where(valid, at_label, torch.zeros_like(at_label))
            ent[s:e] = torch.where(valid, H, torch.zeros_like(H))
        ctx.save_for_backward(flat_h, weight, flat_l)
        ctx.temperature = temperature
        ctx.chunk_size = chunk_size
        ctx.ignore_index = ignore_index
        ctx.hshape = hidden_states.shape
        return lp.view(labels.shape), ent.view(labels.shape)

    @staticmethod
    def backward(ctx, dlog_probs, dentropy):
        if dlog_probs is None and dentropy is None:
            return None, None, None, None, None, None
        flat_h, weight, flat_l = ctx.saved_tensors
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dlp = dlog_probs.reshape(-1).float() if dlog_probs is not None else None
        dent = dentropy.reshape(-1).float() if dentropy is not None else None
        grad_h = torch.zeros_like(flat_h) if need_h else None
        grad_w = torch.zeros_like(weight) if need_w else None
        T_flat = flat_h.shape[0]
        for s in range(0, T_flat, ctx.chunk_size):
            e = min(s + ctx.chunk_size, T_flat)
            h = flat_h[s:e]
            logits = EagerChunkLogProbs._chunk_logits(h, weight, ctx.temperature)
            lab = flat_l[s:e]
            valid = (lab != ctx.ignore_index).float()
            probs = logits.softmax(dim=-1)
            dlogits = torch.zeros_like(probs)
            if dlp is not None:
                onehot = torch.zeros_like(probs).scatter_(
                    -1, lab.clamp(min=0).unsqueeze(-1), 1.0)
                dlogits = dlogits + (dlp[s:e] * valid).unsqueeze(-1) * (onehot - probs)
            if dent is not None:
                logp = logits.log_softmax(dim=-1)
                H = torch.logsumexp(logits, dim=-1) - torch.sum(probs * logits, dim=-1)
                dlogits = dlogits + probs * (logp + H.unsqueeze(-1)) * (
                    -(dent[s:e] * valid).unsqueeze(-1))
            dlogits = dlogits.to(h.dtype)
            if ctx.temperature != 1.0:
                dlogits = dlogits / ctx.temperature
            if need_h:
                grad_h[s:e] = dlogits @ weight
            if need_w:
                grad_w += dlogits.t() @ h
        if need_h:
            grad_h = grad_h.view(ctx.hshape)
        return grad_h, grad_w, None, None, None, None


def _align_logprobs(hidden_states, labels, shift_labels):
    """The reference's three alignment modes (ref chunk_logprobs.py:324-343).
    Returns (hidden, targets, pad): pad says the outputs get one trailing 0."""
    if shift_labels is not None:          # caller-aligned: used as is
        return hidden_states, shift_labels, False
    if get_parallel_state().sp_enabled:   # the SP collator shifted already
        return hidden_states, labels, False
    return (hidden_states[..., :-1, :].contiguous(),
            labels[..., 1:].contiguous(), True)


def _pad_logprobs(log_probs, entropy, pad):
    if pad:
        log_probs = torch.nn.functional.pad(log_probs, (0, 1), value=0.0)
        entropy = torch.nn.functional.pad(entropy, (0, 1), value=0.0)
    return log_probs, entropy


def hip_chunk_logprobs_function(hidden_states, weights, labels,
                                chunk_size: int = 1024,
                                ignore_index: int = IGNORE_INDEX,
                                shift_labels=None, temperature: float = 1.0):
    """Per-token (log_probs, entropy), fp32, shaped like `labels` (or like
    `shift_labels` when given); 0 at ignored positions and at the pad slot."""
    hidden_states, targets, pad = _align_logprobs(hidden_states, labels,
                                                  shift_labels)
    temperature, chunk_size = float(temperature), int(chunk_size)
    ignore_index = int(ignore_index)
    if torch.is_grad_enabled() and (hidden_states.requires_grad
                                    or weights.requires_grad):
        lp, ent = HipChunkLogProbs.apply(hidden_states, weights, targets,
                                         temperature, chunk_size, ignore_index)
    else:
        # nothing to differentiate: no row statistics, nothing saved
        lp, ent, _, _ = _hip_logprobs_chunks(
            hidden_states.reshape(-1, hidden_states.shape[-1]), weights,
            _flat_labels(targets), temperature, chunk_size, ignore_index,
            want_stats=False)
        lp, ent = lp.view(targets.shape), ent.view(targets.shape)
    return _pad_logprobs(lp, ent, pad)


def eager_chunk_logprobs_function(hidden_states, weights, labels,
                                  chunk_size: int = 1024,
                                  ignore_index: int = IGNORE_INDEX,
                                  shift_labels=None, temperature: float = 1.0):
    """Torch-only twin of hip_chunk_logprobs_function (impl "eager", CPU
    tests, GPU baseline)."""
    hidden_states, targets, pad = _align_logprobs(hidden_states, labels,
                                                  shift_labels)
    lp, ent = EagerChunkLogProbs.apply(hidden_states, weights, targets,
                                       float(temperature), int(chunk_size),
                                       int(ignore_index))
    return _pad_logprobs(lp, ent, pad)


# --------------------------------------------------------------------------
# Top-k forward-KL distillation (the teacher_topk_* part of the contract)
# --------------------------------------------------------------------------
def _flat_teacher(teacher_topk_ids, teacher_topk_log_probs, dtype=None):
    K = teacher_topk_ids.shape[-1]
    ids = teacher_topk_ids.reshape(-1, K).to(torch.int64).contiguous()
    tlp = teacher_topk_log_probs.reshape(-1, K)
    if dtype is not None:
        tlp = tlp.to(dtype)
    return ids, tlp.contiguous()


def _hip_topk_chunks(flat_h, weight, flat_l, ids, tlp, temperature, chunk_size,
                     ignore_index, clamp):
    """Chunked lm_head GEMM + vh_logprob_fwd + vh_topk_kl_fwd per chunk.
    Returns fp32 [T] (log_probs, entropy, lse, ent_raw, distill,
    student_mass, teacher_mass)."""
    if flat_h.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise TypeError(
            "the hip top-k distillation path takes bf16 hidden_states and "
            f"weights, got {flat_h.dtype} / {weight.dtype}; bind the slot "
            "'eager' for other dtypes")
    T_flat = flat_h.shape[0]
    parts = []
    for s in range(0, T_flat, chunk_size):
        e = min(s + chunk_size, T_flat)
        logits = torch.matmul(flat_h[s:e], weight.t())
        stats = hip_lib.logprob_fwd(logits, flat_l[s:e], temperature,
                                    ignore_index, want_stats=True)
        kl = hip_lib.topk_kl_fwd(logits, flat_l[s:e], stats[2], ids[s:e],
                                 tlp[s:e], temperature, clamp, ignore_index)
        parts.append(stats + kl)
    if not parts:
        z = torch.zeros(0, dtype=torch.float32, device=flat_h.device)
        return tuple(z.clone() for _ in range(7))
    return tuple(torch.cat(c) for c in zip(*parts))


class HipChunkTopkDistill(torch.autograd.Function):
    """(log_probs, entropy, distill, student_mass, teacher_mass) through the
    lm_head without building [T, V] or any fp32 [chunk, V] tensor.

    Forward keeps hidden/weight/labels, the teacher's ids and fp32 log-probs
    and the two fp32 [T] row statistics; backward re-issues each chunk's
    logits GEMM exactly as forward did and runs vh_topk_distill_bwd (or
    vh_logprob_bwd when distill received no gradient) into one reused bf16
    [chunk, V] buffer."""

    @staticmethod
    def forward(ctx, hidden_states, weight, labels, ids, tlp, temperature,
                chunk_size, ignore_index, clamp):
        ctx.set_materialize_grads(False)
        flat_h = hidden_states.reshape(-1, hidden_states.shape[-1])
        flat_l = _flat_labels(labels)
        lp, ent, lse, raw, dist, sm, tm = _hip_topk_chunks(
            flat_h, weight, flat_l, ids, tlp, temperature, chunk_size,
            ignore_index, clamp)
        ctx.save_for_backward(flat_h, weight, flat_l, ids, tlp, lse, raw)
        ctx.temperature = temperature
        ctx.chunk_size = chunk_size
        ctx.ignore_index = ignore_index
        ctx.clamp = clamp
        ctx.hshape = hidden_states.shape
        sm, tm = sm.view(labels.shape), tm.view(labels.shape)
        ctx.mark_non_differentiable(sm, tm)
        return (lp.view(labels.shape), ent.view(labels.shape),
                dist.view(labels.shape), sm, tm)

    @staticmethod
    def backward(ctx, dlog_probs, dentropy, ddistill, _dsm=None, _dtm=None):
        none = (None,) * 9
        if dlog_probs is None and dentropy is None and ddistill is None:
            return none
        flat_h, weight, flat_l, ids, tlp, lse, raw = ctx.saved_tensors
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_h or need_w):
            return none

        def flat(g):
            return g.reshape(-1).float().contiguous() if g is not None else None

        dlp, dent, ddist = flat(dlog_probs), flat(dentropy), flat(ddistill)
        T_flat, V = flat_h.shape[0], weight.shape[0]
        cs = ctx.chunk_size
        grad_h = torch.empty_like(flat_h) if need_h else None
        grad_w32 = (torch.zeros(weight.shape, dtype=torch.float32,
                                device=weight.device) if need_w else None)
        dlog_buf = flat_h.new_empty((min(cs, T_flat), V))
        for s in range(0, T_flat, cs):
            e = min(s + cs, T_flat)
            h = flat_h[s:e]
            logits = torch.matmul(h, weight.t())
            up = (dlp[s:e] if dlp is not None else None,
                  dent[s:e] if dent is not None else None)
            if ddist is None:
                dlog = hip_lib.logprob_bwd(
                    logits, flat_l[s:e], lse[s:e], raw[s:e], *up,
                    ctx.temperature, ctx.ignore_index,
                    dlogits_out=dlog_buf[:e - s])
            else:
                dlog = hip_lib.topk_distill_bwd(
                    logits, flat_l[s:e], lse[s:e], raw[s:e], ids[s:e],
                    tlp[s:e], *up, ddist[s:e], ctx.temperature, ctx.clamp,
                    ctx.ignore_index, dlogits_out=dlog_buf[:e - s])
            if need_h:
                torch.matmul(dlog, weight, out=grad_h[s:e])
            if need_w:
                grad_w32 += torch.matmul(dlog.t(), h).float()
        grad_w = grad_w32.to(weight.dtype) if need_w else None
        if need_h:
            grad_h = grad_h.reshape(ctx.hshape)
        return (grad_h, grad_w) + (None,) * 7


class EagerChunkTopkDistill(torch.autograd.Function):
    """Torch-only twin of HipChunkTopkDistill; restates the reference's
    chunk_topk_distill op for op (ref chunk_topk_distill.py:145-212,
    :237-331), any dtype, any device. As in EagerChunkLogProbs the
    temperature divides the logits in the input dtype before the fp32
    upcast, dlogits is cast to the input dtype before it is divided and
    dweight accumulates in the weight's dtype; in addition the clamp on the
    teacher and teacher_mass are evaluated in the teacher's dtype. The
    accumulation dtype is fp32, as the reference's, except for fp64 inputs,
    which stay fp64 throughout (what gradcheck runs)."""

    @staticmethod
    def _acc(hidden_states):
        return torch.promote_types(hidden_states.dtype, torch.float32)

    @staticmethod
    def _chunk_logits(h, weight, temperature):
        logits = h @ weight.t()
        if temperature != 1.0:
            logits = logits / temperature
        return logits.to(EagerChunkTopkDistill._acc(h))

    @staticmethod
    def forward(ctx, hidden_states, weight, labels, ids, tlp, temperature,
                chunk_size, ignore_index, clamp):
        ctx.set_materialize_grads(False)
        flat_h = hidden_states.reshape(-1, hidden_states.shape[-1])
        flat_l = _flat_labels(labels)
        T_flat = flat_h.shape[0]
        acc = EagerChunkTopkDistill._acc(flat_h)
        lp = torch.zeros(T_flat, dtype=acc, device=flat_h.device)
        ent, dist, sm, tm = (torch.zeros_like(lp) for _ in range(4))
        for s in range(0, T_flat, chunk_size):
            e = min(s + chunk_size, T_flat)
            logits = EagerChunkTopkDistill._chunk_logits(flat_h[s:e], weight,
                                                      temperature)
            lab = flat_l[s:e]
            valid = lab != ignore_index
            logp = logits.log_softmax(dim=-1)
            at_label = logp.gather(-1, lab.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            probs = logits.softmax(dim=-1)
            H = torch.logsumexp(logits, dim=-1) - torch.sum(probs * logits, dim=-1)
            s_k = logp.gather(-1, ids[s:e])
            t_k = tlp[s:e]
            s_mass = s_k.exp().sum(dim=-1)          # both before any clamp
            t_mass = t_k.exp().sum(dim=-1)
            if clamp is not None:
                s_k = s_k.clamp_min(clamp)
                t_k = t_k.clamp_min(clamp)
            t32 = t_k.to(acc)
            kl = (t32.exp() * (t32 - s_k)).sum(dim=-1)
            zero = torch.zeros_like(kl)
            lp[s:e] = torch.where(valid, at_label, zero)
            ent[s:e] = torch.where(valid, H, zero)
            dist[s:e] = torch.where(valid, kl, zero)
            sm[s:e] = torch.where(valid, s_mass, zero)
            tm[s:e] = torch.where(valid, t_mass.to(acc), zero)
        ctx.save_for_backward(flat_h, weight, flat_l, ids, tlp)
        ctx.temperature = temperature
        ctx.chunk_size = chunk_size
        ctx.ignore_index = ignore_index
        ctx.clamp = clamp
        ctx.hshape = hidden_states.shape
        sm, tm = sm.view(labels.shape), tm.view(labels.shape)
        ctx.mark_non_differentiable(sm, tm)
        return (lp.view(labels.shape), ent.view(labels.shape),
                dist.view(labels.shape), sm, tm)

    @staticmethod
    def backward(ctx, dlog_probs, dentropy, ddistill, _dsm=None, _dtm=None):
        none = (None,) * 9
        if dlog_probs is None and dentropy is None and ddistill is None:
            return none
        flat_h, weight, flat_l, ids, tlp = ctx.saved_tensors
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]

        acc = EagerChunkTopkDistill._acc(flat_h)

        def flat(g):
            return g.reshape(-1).to(acc) if g is not None else None

        dlp, dent, ddist = flat(dlog_probs), flat(dentropy), flat(ddistill)
        grad_h = torch.zeros_like(flat_h) if need_h else None
        grad_w = torch.zeros_like(weight) if need_w else None
        T_flat = flat_h.shape[0]
        for s in range(0, T_flat, ctx.chunk_size):
            e = min(s + ctx.chunk_size, T_flat)
            h = flat_h[s:e]
            logits = EagerChunkTopkDistill._chunk_logits(h, weight, ctx.temperature)
            lab = flat_l[s:e]
            valid = (lab != ctx.ignore_index).to(acc)
            probs = logits.softmax(dim=-1)
            dlogits = torch.zeros_like(probs)
            if dlp is not None:
                onehot = torch.zeros_like(probs).scatter_(
                    -1, lab.clamp(min=0).unsqueeze(-1), 1.0)
                dlogits = dlogits + (dlp[s:e] * valid).unsqueeze(-1) * (onehot - probs)
            if dent is not None:
                logp = logits.log_softmax(dim=-1)
                H = torch.logsumexp(logits, dim=-1) - torch.sum(probs * logits, dim=-1)
                dlogits = dlogits + probs * (logp + H.unsqueeze(-1)) * (
                    -(dent[s:e] * valid).unsqueeze(-1))
            if ddist is not None:
                # only s_k depends on the logits; where the clamp holds s_k
                # at its floor the entry has no gradient
                if ctx.clamp is not None:
                    s_k = logits.log_softmax(dim=-1).gather(-1, ids[s:e])
                    w_k = tlp[s:e].clamp_min(ctx.clamp).to(acc).exp() * (
                        s_k >= ctx.clamp).to(acc)
                else:
                    w_k = tlp[s:e].to(acc).exp()
                sparse = torch.zeros_like(probs).scatter_add_(-1, ids[s:e], w_k)
                m_eff = w_k.sum(dim=-1, keepdim=True)
                dlogits = dlogits + (ddist[s:e] * valid).unsqueeze(-1) * (
                    -sparse + m_eff * probs)
            dlogits = dlogits.to(h.dtype)
            if ctx.temperature != 1.0:
                dlogits = dlogits / ctx.temperature
            if need_h:
                grad_h[s:e] = dlogits @ weight
            if need_w:
                grad_w += dlogits.t() @ h
        if need_h:
            grad_h = grad_h.view(ctx.hshape)
        return (grad_h, grad_w) + (None,) * 7


def _align_topk(hidden_states, labels, shift_labels, teacher_topk_ids,
                teacher_topk_log_probs):
    """_align_logprobs plus the teacher tensors (ref chunk_topk_distill.py:
    382-398): they come aligned with the labels, so the default mode drops
    their first slot along with the labels'."""
    hidden_states, targets, pad = _align_logprobs(hidden_states, labels,
                                                  shift_labels)
    if pad:
        teacher_topk_ids = teacher_topk_ids[..., 1:, :]
        teacher_topk_log_probs = teacher_topk_log_probs[..., 1:, :]
    return hidden_states, targets, teacher_topk_ids, teacher_topk_log_probs, pad


def _pad_topk(outs, pad):
    """One trailing 0 on all five; the masses are detached again after it."""
    if not pad:
        return outs
    lp, ent, dist, sm, tm = (torch.nn.functional.pad(t, (0, 1), value=0.0)
                             for t in outs)
    return lp, ent, dist, sm.detach(), tm.detach()


def hip_chunk_topk_distill_function(hidden_states, weights, labels,
                                    teacher_topk_ids, teacher_topk_log_probs,
                                    chunk_size: int = 1024,
                                    ignore_index: int = IGNORE_INDEX,
                                    shift_labels=None,
                                    temperature: float = 1.0,
                                    log_prob_min_clamp: float | None = None):
    """Top-k forward-KL distillation on the student's lm_head: per token
    (log_probs, entropy, distillation_losses, student_mass, teacher_mass),
    fp32, shaped like `labels` (or `shift_labels`), 0 at ignored positions
    and at the pad slot. The first three carry gradients to hidden_states
    and weights; the two masses are metrics (requires_grad=False).

    bf16 hidden_states / weights only. teacher_topk_log_probs of any float
    dtype are upcast once to fp32 [T, K], and everything downstream runs on
    those fp32 values. With bf16 teacher log-probs this differs from the
    reference, which clamps them and sums teacher_mass in bf16 (one bf16
    rounding per partial sum, up to ~K * 2^-9 relative): here the clamp and
    the sum are fp32, so teacher_mass is the more accurate of the two and
    the results agree only to bf16 precision in that field. The distillation
    term itself is fp32 in both."""
    K = teacher_topk_ids.shape[-1]
    if not 1 <= K <= hip_lib.TOPK_MAX:
        raise ValueError(
            f"the hip top-k distillation kernels take 1 <= K <= "
            f"{hip_lib.TOPK_MAX}, got K = {K}; bind the slot 'eager' "
            "(eager_chunk_topk_distill_function) for a wider teacher")
    hidden_states, targets, t_ids, t_lp, pad = _align_topk(
        hidden_states, labels, shift_labels, teacher_topk_ids,
        teacher_topk_log_probs)
    temperature, chunk_size = float(temperature), int(chunk_size)
    ignore_index = int(ignore_index)
    clamp = None if log_prob_min_clamp is None else float(log_prob_min_clamp)
    ids, tlp = _flat_teacher(t_ids, t_lp, torch.float32)
    if torch.is_grad_enabled() and (hidden_states.requires_grad
                                    or weights.requires_grad):
        outs = HipChunkTopkDistill.apply(hidden_states, weights, targets, ids,
                                         tlp, temperature, chunk_size,
                                         ignore_index, clamp)
    else:
        # nothing to differentiate: nothing saved
        lp, ent, _, _, dist, sm, tm = _hip_topk_chunks(
            hidden_states.reshape(-1, hidden_states.shape[-1]), weights,
            _flat_labels(targets), ids, tlp, temperature, chunk_size,
            ignore_index, clamp)
        outs = tuple(t.view(targets.shape) for t in (lp, ent, dist, sm, tm))
    return _pad_topk(outs, pad)


def eager_chunk_topk_distill_function(hidden_states, weights, labels,
                                      teacher_topk_ids, teacher_topk_log_probs,
                                      chunk_size: int = 1024,
                                      ignore_index: int = IGNORE_INDEX,
                                      shift_labels=None,
                                      temperature: float = 1.0,
                                      log_prob_min_clamp: float | None = None):
    """Torch-only twin of hip_chunk_topk_distill_function (impl "eager", CPU
    tests, GPU baseline); any dtype, any K."""
    hidden_states, targets, t_ids, t_lp, pad = _align_topk(
        hidden_states, labels, shift_labels, teacher_topk_ids,
        teacher_topk_log_probs)
    ids, tlp = _flat_teacher(t_ids, t_lp)
    outs = EagerChunkTopkDistill.apply(
        hidden_states, weights, targets, ids, tlp, float(temperature),
        int(chunk_size), int(ignore_index), log_prob_min_clamp)
    return _pad_topk(outs, pad)


def hip_causal_lm_loss(hidden_states=None, weights=None, labels=None,
                       vocab_size=None, num_items_in_batch=None,
                       ignore_index=IGNORE_INDEX, shift_labels=None,
                       chunk_size: int | None = None,
                       return_log_probs: bool = False,
                       temperature: float = 1.0,
                       teacher_topk_ids=None, teacher_topk_log_probs=None,
                       **kwargs):
    """ForCausalLMLoss-shaped entry returning (loss, logits|None, aux|None).

    Causal shift applied here unless SP pre-shifted the labels in the
    collator (ref __init__.py:184-195). With return_log_probs=True the loss
    is skipped and the third slot carries FusedLinearAuxOutput(log_probs,
    entropy) (ref __init__.py:130-177); chunk_size then defaults to 1024,
    on the loss path to 2048."""
    assert hidden_states is not None and weights is not None
    if teacher_topk_ids is not None or teacher_topk_log_probs is not None:
        raise NotImplementedError(
            "top-k distillation (teacher_topk_ids / teacher_topk_log_probs) "
            "is not routed through hip_causal_lm_loss; call "
            "hip_chunk_topk_distill_function, or the model with "
            "return_log_probs=True and both teacher tensors")
    if return_log_probs:
        log_probs, entropy = hip_chunk_logprobs_function(
            hidden_states, weights, labels,
            chunk_size=1024 if chunk_size is None else chunk_size,
            ignore_index=ignore_index, shift_labels=shift_labels,
            temperature=temperature)
        return None, None, FusedLinearAuxOutput(log_probs=log_probs,
                                                entropy=entropy)
    if chunk_size is None:
        chunk_size = 2048
    sp_enabled = get_parallel_state().sp_enabled
    orig_labels = labels
    if not sp_enabled:
        labels = labels[..., 1:].contiguous()
        hidden_states = hidden_states[..., :-1, :].contiguous()
    loss = HipChunkCE.apply(hidden_states, weights, labels, chunk_size)
    if sp_enabled:
        num_valid = (orig_labels != ignore_index).sum()
        loss = reduce_sequence_parallel_loss(loss, num_valid)
    return loss, None, None


KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip", op_name="cross_entropy_loss", variant="causal",
        factory=lambda: hip_causal_lm_loss,
        hardware=HardwareRequirement(device_type="gpu"),
        description="gfx950 chunked fused-linear CE (vh_ce_fwd + hipBLASLt chunks); "
                    "return_log_probs via vh_logprob_fwd/_bwd",
    )
)
