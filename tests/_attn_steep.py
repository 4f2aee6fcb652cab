"""Steep attention inputs, and a host-side model of the prefill kernels' deferred softmax rescale (a plain helper module).

The prefill kernels keep a per-row reference that the scores are measured against, and move it only when a score outgrows it:
  "lazy"  fa3_fwd5_body.inc (every form) and the K-prescaled fa3_fwd3_body.inc: reference = row maximum of the tile at the last
          move + MARGIN (5 in bf16, 2 in fp16, base-2 units); a row moves when some P = 2^(score - reference) >= 2; a carried
          row starts from lse_in with no margin;
  "fwd3"  fa3_fwd3_body.inc `update`: a score more than THR = 6 above the reference, new reference = the running row maximum;
  "fwd1"  fa3_fwd_kernel.h: the same threshold.
The two threshold rules test once per wave (64 / 32 consecutive query rows): when one row of a wave triggers, every row of
the wave raises its reference to its running maximum, so rows below the threshold move too, by a smaller step.

steep_inputs() draws q / k / v on which rows do move after their first tile (randn data at scale 1/sqrt(D) never does),
move_plan() emulates the three triggers on fp64 scores, lazy_chain() is a plain fp32 tiled chain with 16-bit P under the same
rules -- no code shared with the kernels -- that takes an injected defect, and CASES is the table of GPU launches
tests/test_gpu_attention_steep.py makes; tests/test_attn_steep_host.py proves the input conditions for every one of them.
reference() / judge() are the fp64 reference of a case and the judgement both test files apply: the output rows by
_attn_check.check at the unchanged BARS of the route's family, lse by the absolute bar lse_bar().
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import _attn_check as ac

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
TILE = 64
THR = 6.0
MARGIN = {torch.bfloat16: 5.0, torch.float16: 2.0}
WAVE_ROWS = {"lazy": None, "fwd3": 64, "fwd1": 32}
NEG_FILL = -1e9          # oracle.attention.NEG_FILL: keep-masked keys, and causal-excluded keys under a user mask
ADD_MASK_FLOOR = -1e30
F8 = torch.float8_e4m3fn
RESERVED = 8             # trailing head dims the profiles own
DEFECTS = ("alpha_dropped", "alpha_row16", "next_not_shifted", "trigger_ignored")

def rule_of(route: str) -> str:
    if route.startswith("fwd5") or route == "fwd3_kpre":
        return "lazy"
    return "fwd3" if route == "fwd3" else "fwd1"


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def steep_inputs(profile, dtype, *, Sq, Sk, D, scale, B=1, H=2, Hkv=None, kpre=False, h=None, first_spike_tile=2,
                 spread=1, step=8.0, q_amp=None, seed=0):
    """16-bit q [B,Sq,H,D], k / v [B,Sk,Hkv,D] (CPU) of one profile; `scale` is the softmax scale of the launch.  The random
    part of q is 0.5 * randn, of k and v randn; the last RESERVED dims of q and k carry the profile:
      spikes   query row i holds a in reserved dim (i + i//16 + i//32) % 8; in every 64-key tile t >= first_spike_tile the
               keys at in-tile offsets 17 and 40 hold a in dims (3 t) % 8 and (3 t + 5) % 8 (and the `spread` - 1 dims
               after each, modulo 8): a^2 * scale * log2(e) = h;
      rising   reserved dim 7 adds step * (j // 64) base-2 units to the score of key j (q holds q_amp there);
      falling  ... subtracts it.
    kpre: k is K * scale * log2(e), scaled in fp32 before its one rounding (the reference then uses scale ln 2)."""
    Hkv = H if Hkv is None else Hkv
    g = torch.Generator().manual_seed(seed * 7919 + Sq * 31 + Sk * 17 + D + {"spikes": 0, "rising": 1, "falling": 2}[profile])
    q = torch.randn(B, Sq, H, D, generator=g) * 0.5
    k = torch.randn(B, Sk, Hkv, D, generator=g)
    v = torch.randn(B, Sk, Hkv, D, generator=g)
    q[..., D - RESERVED:] = 0
    k[..., D - RESERVED:] = 0
    c2 = scale * LOG2E
    i = torch.arange(Sq)
    j = torch.arange(Sk)
    t = j // TILE
    if profile == "spikes":
        a = math.sqrt(h / c2)
        q[:, i, :, D - RESERVED + (i + i // 16 + i // 32) % 8] = a
        for off, dim in ((17, (3 * t) % 8), (40, (3 * t + 5) % 8)):
            sel = (j % TILE == off) & (t >= first_spike_tile)
            for extra in range(spread):
                k[:, j[sel], :, D - RESERVED + (dim[sel] + extra) % 8] = a
    else:
        ntile = (Sk + TILE - 1) // TILE
        if q_amp is None:  # a power of two that keeps the key column at or below 16 (inside e4m3's range at k_scale 0.05)
            q_amp = 2.0 ** math.ceil(math.log2(max(step * ntile / (16.0 * c2), 1.0)))
        col = (step / (q_amp * c2)) * t.float()
        q[..., D - 1] = q_amp
        k[..., D - 1] = (col if profile == "rising" else -col)[None, :, None]
    if kpre:
        k = k * c2
    return q.to(dtype), k.to(dtype), v.to(dtype)


def quant_kv8(x, s):
    """The cache-write formula on the CPU (test_gpu_kv8._quant_ref): x 16-bit, s the fp32 scale as a python float."""
    return (x.float() * (torch.tensor(1.0) / torch.tensor(s, dtype=torch.float32))).clamp(-448, 448).to(F8)


def visibility(Sq, Sk, *, causal=False, off=0, window=(-1, -1)):
    """bool [Sq,Sk]: query i sees key j; off = q_offset - k_offset; window = (left, right), -1 unbounded."""
    i = torch.arange(Sq).view(Sq, 1) + off
    j = torch.arange(Sk).view(1, Sk)
    left, right = window
    vis = torch.ones(Sq, Sk, dtype=torch.bool)
    if causal or right >= 0:
        vis &= j <= i + (0 if causal else right)
    if left >= 0:
        vis &= j >= i - left
    return vis


def scores_base2(q, k, c2, *, vis=None):
    """fp64 [B,H,Sq,Sk] base-2 scores of q [B,Sq,H,D], k [B,Sk,Hkv,D] (any float dtype): q.k * c2, hidden keys (vis false)
    -inf."""
    H, Hkv = q.shape[2], k.shape[2]
    kd = k.double().repeat_interleave(H // Hkv, dim=2)
    s = torch.einsum("bshd,bkhd->bhsk", q.double(), kd) * c2
    if vis is not None:
        s = s.masked_fill(~vis, float("-inf"))
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the triggers on fp64 scores
# ---------------------------------------------------------------------------------------------------------------------
def _wave_any(x, wave_rows):
    """any() over each run of wave_rows consecutive query rows (dim -1 of x), broadcast back."""
    if wave_rows is None:
        return x
    n = x.shape[-1]
    pad = (-n) % wave_rows
    y = torch.nn.functional.pad(x, (0, pad)).view(*x.shape[:-1], -1, wave_rows).any(-1, keepdim=True)
    return y.expand(*x.shape[:-1], (n + pad) // wave_rows, wave_rows).reshape(*x.shape[:-1], n + pad)[..., :n]


def move_plan(scores, rule, *, dtype=torch.bfloat16, tile=TILE, first_tile=0, carried_lse=None):
    """Emulate a rule's trigger on fp64 base-2 scores [..., Sq, Sk] (-inf = hidden key), tiles of `tile` keys from key
    first_tile * tile on (earlier keys must be hidden).  carried_lse [..., Sq] (natural units, -inf = nothing carried):
    the rows continue from it, without a margin.  Returns a dict:
      moves  bool [..., Sq, T]: the row's reference moves at tile t with O and L rescaled (alpha != 1): not the first
             visible tile of a fresh row;
      sees   bool [..., Sq, T]: the row sees a key of tile t;
      share  [..., Sq]: over the row's moves, the largest share of the weight it has accumulated by the end of these scores
             (a carried row's carry included) that was accumulated before the move."""
    assert rule in WAVE_ROWS
    Sk = scores.shape[-1]
    T = (Sk + tile - 1) // tile
    lead = scores.shape[:-1]
    ref = torch.full(lead, float("-inf"), dtype=torch.float64)   # lazy: the reference; threshold rules: the running maximum
    if carried_lse is not None:
        ref = carried_lse.double() * LOG2E
    carried = ref.clone()                                        # log2 of the carried weight
    fresh = torch.isinf(ref)
    moves = torch.zeros(*lead, T, dtype=torch.bool)
    sees = torch.zeros(*lead, T, dtype=torch.bool)
    wave = WAVE_ROWS[rule]
    for t in range(first_tile, T):
        mx = scores[..., t * tile:(t + 1) * tile].amax(-1)
        vis = ~torch.isinf(mx)
        sees[..., t] = vis
        if rule == "lazy":
            need = vis & (mx - ref >= 1.0) & ~fresh
            moves[..., t] = need
            ref = torch.where(need | (fresh & vis), mx + MARGIN[dtype], ref)
        else:
            trig = vis & ((mx > ref + THR) | fresh)
            anyw = _wave_any(trig, wave)
            moves[..., t] = anyw & vis & ~fresh & (mx > ref)
            ref = torch.where(anyw & vis, torch.maximum(ref, mx), ref)
        fresh = fresh & ~vis
    # weights relative to the row's final maximum (carry included)
    top = torch.maximum(scores.amax(-1), carried)
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    w = torch.exp2(scores - top[..., None])   # (2^-inf = 0 for hidden keys)
    cw = torch.exp2(carried - top)
    total = w.sum(-1) + cw
    before = cw.clone()
    share = torch.zeros(lead, dtype=torch.float64)
    for t in range(T):
        share = torch.where(moves[..., t], torch.maximum(share, before / total.clamp_min(1e-300)), share)
        before = before + w[..., t * tile:(t + 1) * tile].sum(-1)
    return {"moves": moves, "sees": sees, "share": share}


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 chain with 16-bit P
# ---------------------------------------------------------------------------------------------------------------------
def lazy_chain(q, k, v, c2, dtype, rule, *, bias=None, carried=None, defect=None, tile=TILE):
    """A plain fp32 chain over 64-key tiles: q [B,Sq,H,D], k / v [B,Sk,Hkv,D] (the values the kernel multiplies: 16-bit, or
    the dequantised fp8 cache), c2 the factor from q.k to base-2 units.  bias [B|1,H|1,Sq,Sk] base-2, added to the scores:
    -inf hides a key (build it from scores_base2 of zeros).  carried = (o fp32 [B,Sq,H,D], lse fp32 [B,H,Sq]).
    Each tile's P = 2^(score - reference) is rounded to `dtype` before it is summed and multiplied with V; the reference
    follows `rule`.  defect: one of DEFECTS, or None.  Returns (o fp32 [B,Sq,H,D], lse
    fp32 [B,H,Sq]); rows that saw no key: (0, -inf)."""
    assert rule in WAVE_ROWS and (defect is None or defect in DEFECTS)
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
    vf = v.float().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
    ninf = torch.full((B, H, Sq), float("-inf"))
    ref = ninf.clone()
    O = torch.zeros(B, H, Sq, D)
    L = torch.zeros(B, H, Sq)
    if carried is not None:
        co, cl = carried
        has = ~torch.isinf(cl)
        ref = torch.where(has, cl.float() * LOG2E, ninf)
        L = has.float()
        O = torch.where(has[..., None], co.float().permute(0, 2, 1, 3), O)
    fresh = torch.isinf(ref)
    pend = torch.zeros(B, H, Sq)  # next_not_shifted: what the next tile's scores were not shifted by
    wave = WAVE_ROWS[rule]
    c2 = torch.tensor(c2, dtype=torch.float32)
    margin = MARGIN[dtype]
    for t in range((Sk + tile - 1) // tile):
        lo, hi = t * tile, min((t + 1) * tile, Sk)
        s = (qf @ kf[:, :, lo:hi].transpose(-1, -2)) * c2
        if bias is not None:
            s = s + bias[..., lo:hi].float()
        s = s + pend[..., None]
        pend = torch.zeros_like(pend)
        mx = s.amax(-1)
        vis = ~(torch.isinf(mx) & (mx < 0))
        if rule == "lazy":
            need = vis & ~fresh & (mx - ref >= 1.0)
            new = torch.where(need | (fresh & vis), mx + margin, ref)
        else:
            trig = vis & (fresh | (mx > ref + THR))
            need = _wave_any(trig, wave) & vis & ~fresh & (mx > ref)
            new = torch.where(_wave_any(trig, wave) & vis, torch.maximum(ref, mx), ref)
        if defect == "trigger_ignored":
            new = torch.where(need, ref, new)
            need = torch.zeros_like(need)
        delta = torch.where(need, new - ref, torch.zeros_like(ref))
        alpha = torch.exp2(-delta)
        if defect == "alpha_dropped":
            alpha = torch.ones_like(alpha)
        elif defect == "alpha_row16":
            idx = torch.arange(Sq) ^ 16
            alpha = torch.where(idx < Sq, alpha[..., idx.clamp_max(Sq - 1)], torch.ones_like(alpha))
        elif defect == "next_not_shifted" and t > 0:
            pend = delta
        O = O * alpha[..., None]
        L = L * alpha
        ref = new
        fresh = fresh & ~vis
        rs = torch.where(torch.isinf(ref), torch.zeros_like(ref), ref)
        p = torch.exp2(s - rs[..., None]).to(dtype).float()
        L = L + p.sum(-1)
        O = O + p @ vf[:, :, lo:hi]
    live = ~fresh
    o = torch.where(live[..., None], O / torch.where(live, L, torch.ones_like(L))[..., None], torch.zeros_like(O))
    lse = torch.where(live, (ref + torch.log2(torch.where(live, L, torch.ones_like(L)))) * LN2, ninf)
    return o.permute(0, 2, 1, 3).contiguous(), lse


# ---------------------------------------------------------------------------------------------------------------------
# the table of GPU launches
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    group: str                      # dense / carry / varlen / paged / kv8 / window_dense / window_varlen / window_paged
    route: str                      # what the *_route query must answer
    D: int
    profile: str
    causal: bool = False
    scale: Optional[float] = None   # None: K-prescaled (scale 1/sqrt(D) folded into K)
    Sq: int = 300
    Sk: int = 600
    B: int = 1
    H: int = 2
    Hkv: int = 2
    oblk: bool = False
    mask: Optional[str] = None      # "add" / "keep"
    splits: tuple = ()              # carry: cumulative shard ends
    lens_q: tuple = ()              # varlen / paged
    lens_k: tuple = ()
    bs: int = 64
    window: tuple = (-1, -1)

    @property
    def kpre(self):
        return self.scale is None

    @property
    def rule(self):
        return rule_of(self.route)

    @property
    def id(self):
        sc = "kpre" if self.kpre else f"s{self.scale:.3g}"
        extra = f"-bs{self.bs}" if self.group in ("paged", "kv8", "window_paged") else ""
        gqa = f"-gqa{self.H}/{self.Hkv}" if self.H != self.Hkv else ""
        return f"{self.group}-{self.route}-D{self.D}-{self.profile}-{'causal' if self.causal else 'full'}-{sc}{extra}{gqa}"


def _dense_cases():
    out = []
    routes = [("fwd5", 64, 0.2, {}), ("fwd5", 40, 1.7 / math.sqrt(40), {}), ("fwd5_kpre", 64, None, {}),
              ("fwd5_kpre_oblk", 64, None, dict(oblk=True)), ("fwd3", 128, 0.2, {}), ("fwd3", 96, 1.7 / math.sqrt(96), {}),
              ("fwd3_kpre", 96, None, {}), ("fwd1", 64, 0.2, dict(Sq=100)), ("fwd1", 128, 1.7 / math.sqrt(128), dict(Sq=100)),
              ("fwd1_add", 64, 0.2, dict(mask="add")), ("fwd1_keep", 64, 1.7 / 8, dict(mask="keep"))]
    for route, D, scale, kw in routes:
        for profile in ("spikes", "rising", "falling"):
            for causal in (False, True):
                out.append(Case("dense", route, D, profile, causal, scale, **kw))
    out.append(Case("dense", "fwd5", 64, "spikes", False, 1.7 / 8, H=4, Hkv=2))
    out.append(Case("dense", "fwd3", 128, "spikes", False, 1.7 / math.sqrt(128), H=4, Hkv=2))
    out.append(Case("dense", "fwd1", 64, "spikes", False, 1.7 / 8, Sq=100, H=4, Hkv=2))
    return out


_LENS_Q = (300, 77, 600)


def _cases():
    out = _dense_cases()
    for route, D, scale, Sq in (("fwd5_kpre_carry", 64, None, 300), ("fwd3", 128, 0.2, 300), ("fwd1", 64, 1.7 / 8, 100)):
        for profile in ("spikes", "rising"):
            out.append(Case("carry", route, D, profile, False, scale, Sq=Sq, B=2, splits=(130, 333, 600)))
    for route, D, scale in (("fwd5", 64, 0.2), ("fwd3", 128, 1.7 / math.sqrt(128))):
        for profile in ("spikes", "rising", "falling"):
            for causal in (False, True):
                out.append(Case("varlen", route, D, profile, causal, scale, lens_q=_LENS_Q, lens_k=_LENS_Q))
    ctx = tuple(n + p for n, p in zip(_LENS_Q, (300, 128, 41)))  # a context prefix in front of every chunk: Lk > Lq
    for route, D, scale in (("fwd5", 64, 1.7 / 8), ("fwd3", 128, 0.2)):
        for bs in (64, 128):  # (the paged kernels take block sizes that are multiples of 64)
            for profile in ("spikes", "rising", "falling"):
                out.append(Case("paged", route, D, profile, True, scale, lens_q=_LENS_Q, lens_k=ctx, bs=bs))
        for profile in ("spikes", "rising", "falling"):
            out.append(Case("kv8", route, D, profile, True, scale, lens_q=_LENS_Q, lens_k=ctx, bs=64))
    for route, D, scale in (("fwd5", 64, 0.2), ("fwd3", 128, 1.7 / math.sqrt(128))):
        w = dict(causal=True, window=(100, 0))
        for profile in ("spikes", "rising"):
            out.append(Case("window_dense", route, D, profile, scale=scale, **w))
            out.append(Case("window_varlen", route, D, profile, scale=scale, lens_q=_LENS_Q, lens_k=_LENS_Q, **w))
            out.append(Case("window_paged", route, D, profile, scale=scale, lens_q=_LENS_Q, lens_k=ctx, bs=64, **w))
    return out


CASES = _cases()
KV8_SCALES = (0.05, 0.08)


@dataclass
class Problem:
    """One (sequence, shard) of a case as the kernel sees it: 16-bit q, k, v (CPU; k / v as handed to the launch, or for the
    fp8 cache the 16-bit tensors handed to the cache write); kk / vv: the float values the kernel multiplies (k / v, or the
    dequantised cache); c2: q.kk -> base-2 units; bias: base-2 [B|1,H|1,Sq,Sk] with -inf for hidden keys, or None; ref_scale:
    the softmax scale of the fp64 reference over (q, kk, vv); first_tile: the first 64-key tile any row sees."""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    kk: torch.Tensor
    vv: torch.Tensor
    c2: float
    ref_scale: float
    bias: Optional[torch.Tensor] = None
    first_tile: int = 0
    extra: dict = field(default_factory=dict)


def bulk_sigma(D, c2):
    """Standard deviation, in base-2 units, of the random part of a score: 0.5 * randn(D - 8) . randn(D - 8) * c2."""
    return 0.5 * math.sqrt(D - RESERVED) * c2


def spike_h(case, dtype):
    """The spike height of a case in base-2 units, rounded up to half a unit: what the rule asks above the row's state
    before the spike, and nothing larger.  A row's maximum over the few hundred keys before its first spike lies about
    3 sigma above 0 (3.5 sigma clears most rows; the others simply do not move), and the spike must exceed it by MARGIN
    + 1 (lazy) or THR.  A carried row's state is its lse instead: log2 of the key count (all of case.Sk for the last
    shard) plus sigma^2 ln2 / 2 for the mean of 2^score; the lazy rule asks 1 above it, the threshold rules THR."""
    c2 = 1.0 / math.sqrt(case.D) * LOG2E if case.kpre else case.scale * LOG2E
    sd = bulk_sigma(case.D, c2)
    ask = MARGIN[dtype] + 1.0 if case.rule == "lazy" else THR
    if case.group == "carry":
        h = math.log2(case.Sk) + 0.5 * LN2 * sd * sd + (1.0 if case.rule == "lazy" else THR) + 0.5
    else:
        h = 3.5 * sd + ask
    return math.ceil(2.0 * h) / 2.0


def rising_step(case, dtype):
    """The base-2 units a 64-key tile adds in `rising`: 8, or what makes EVERY row move at every tile where that is more.
    A row may see one key of an edge tile (causal, window) and all 64 of the tile before: that key can lie 6 sigma below
    the other tile's maximum, and the step must still clear MARGIN + 1 (lazy) or THR."""
    c2 = 1.0 / math.sqrt(case.D) * LOG2E if case.kpre else case.scale * LOG2E
    ask = MARGIN[dtype] + 1.0 if case.rule == "lazy" else THR
    return max(8.0, math.ceil(2.0 * (ask + 6.0 * bulk_sigma(case.D, c2))) / 2.0)


def _masks(case, B, H, Sq, Sk, g):
    """(keep, add) 4-D CPU masks of a masked dense case, else (None, None)."""
    if case.mask == "add":  # test_additive_masks' b1qk form
        add = torch.randn(B, 1, Sq, Sk, generator=g) * 2
        add[..., ::5] = -1e4
        return None, add
    if case.mask == "keep":
        keep = (torch.rand(B, H, Sq, Sk, generator=g) > 0.3).to(torch.uint8)
        keep[..., 0] = 1
        return keep, None
    return None, None


def build(case, dtype):
    """The case's problems, in launch order: one per dense launch, per sequence of a varlen / paged launch, or one for the
    whole carry (its shards are cut from it at case.splits).  Deterministic: the host tests and the GPU tests call it with
    the same arguments and get the same tensors."""
    D = case.D
    scale = (1.0 / math.sqrt(D)) if case.kpre else case.scale
    c2 = 1.0 if case.kpre else scale * LOG2E
    ref_scale = LN2 if case.kpre else scale
    short = case.causal  # (a carry keeps its first shard free of spikes: the second shard's first tile holds the first)
    # a 100-key window shows a row at most two spiked tiles after its first: two classes per spike key there, so that
    # a quarter of the rows still meets one
    kw = dict(D=D, scale=scale, H=case.H, Hkv=case.Hkv, kpre=case.kpre, h=spike_h(case, dtype),
              first_spike_tile=1 if short else 2, spread=2 if case.window[0] >= 0 else 1,
              step=rising_step(case, dtype) if case.profile == "rising" else 8.0)
    probs = []
    if case.group in ("dense", "carry", "window_dense"):
        q, k, v = steep_inputs(case.profile, dtype, Sq=case.Sq, Sk=case.Sk, B=case.B, **kw)
        off = case.Sk - case.Sq if case.causal else 0
        g = torch.Generator().manual_seed(case.Sq + case.Sk + D)
        keep, add = _masks(case, case.B, case.H, case.Sq, case.Sk, g)
        vis = visibility(case.Sq, case.Sk, causal=case.causal, off=off, window=case.window)
        if case.mask is None:
            bias = scores_base2(torch.zeros(1, case.Sq, 1, 1), torch.zeros(1, case.Sk, 1, 1), 1.0, vis=vis)
        else:  # under a user mask causal-excluded keys get the finite fill (include/mio_hip.h)
            fill = ~vis[None, None] if keep is None else (~vis[None, None] | (keep == 0))
            z = torch.zeros(case.B, case.H, case.Sq, case.Sk, dtype=torch.float64)
            bias = torch.where(fill, torch.full_like(z, NEG_FILL * LOG2E), z)
            if add is not None:
                bias = bias + add.double().clamp_min(ADD_MASK_FLOOR) * LOG2E
        probs.append(Problem(q, k, v, k, v, c2, ref_scale, bias, _first_tile(off, case.window),
                             extra=dict(off=off, keep=keep, add=add)))
        return probs
    for b, (Lq, Lk) in enumerate(zip(case.lens_q, case.lens_k)):
        q, k, v = steep_inputs(case.profile, dtype, Sq=Lq, Sk=Lk, seed=b + 1, **kw)
        kk, vv = k, v
        if case.group == "kv8":  # the reference and the chain run over the dequantised cache
            ks, vs = KV8_SCALES
            kk, vv = quant_kv8(k, ks).double() * ks, quant_kv8(v, vs).double() * vs
        vis = visibility(Lq, Lk, causal=case.causal, off=Lk - Lq, window=case.window)
        bias = scores_base2(torch.zeros(1, Lq, 1, 1), torch.zeros(1, Lk, 1, 1), 1.0, vis=vis)
        probs.append(Problem(q, k, v, kk, vv, c2, ref_scale, bias, _first_tile(Lk - Lq, case.window), extra=dict(off=Lk - Lq)))
    return probs


def _first_tile(off, window):
    return max(off - window[0], 0) // TILE if window[0] >= 0 else 0


def shards(case, prob):
    """(lo, hi) key ranges of the launches over one problem: the carry's splits, else everything."""
    if case.group != "carry":
        return [(0, prob.kk.shape[1])]
    return list(zip((0,) + case.splits[:-1], case.splits))


def plan(case, dtype, prob):
    """move_plan over one problem (a carry: shard by shard, each continued from the exact lse of the keys before it, the tile
    axes concatenated) plus its fp64 base-2 scores."""
    s = scores_base2(prob.q, prob.kk, prob.c2)
    if prob.bias is not None:
        s = s + prob.bias
    parts = []
    for lo, hi in shards(case, prob):
        carried = torch.logsumexp(s[..., :lo] * LN2, dim=-1) if lo > 0 else None
        parts.append(move_plan(s[..., lo:hi], case.rule, dtype=dtype, first_tile=prob.first_tile if lo == 0 else 0,
                               carried_lse=carried))
    # a shard's shares are of the weight at the shard's end: rescale to the weight at the end of all keys
    tot = torch.logsumexp(s * LN2, dim=-1)
    sh = [p["share"] * torch.exp(torch.logsumexp(s[..., :hi] * LN2, dim=-1) - tot).nan_to_num(0.0)
          for p, (lo, hi) in zip(parts, shards(case, prob))]
    return {"moves": torch.cat([p["moves"] for p in parts], -1), "sees": torch.cat([p["sees"] for p in parts], -1),
            "share": torch.stack(sh).amax(0), "scores": s}


def describe_row(pl, b, h, i):
    """'moved at tiles [..]' / 'never moved' of one row of a plan: for failure messages."""
    t = pl["moves"][b, h, i].nonzero().flatten().tolist()
    return f"row (b {b}, head {h}, query {i}): " + (f"moves at tiles {t}, share {pl['share'][b, h, i]:.3f}" if t else "never moves")


def conditions(case, dtype, share_bar=0.1):
    """The input statistics tests/test_attn_steep_host.py bounds, over every problem of the case:
      live / moved       rows that see a key / whose reference moves with a rescale;
      mixed              share of 16-row groups that hold, at some tile, a row that moves and a row that sees the tile and
                         does not;
      carried            share of the moved rows with >= share_bar of their weight accumulated before a move;
      twice              share of the rows that see three or more tiles and move at least twice;
      late               moves after a row's first visible tile (the count `falling` must keep at zero: every move is one);
      faint              smallest share, over the rows that see >= 512 keys, of keys below 2^-24 of the row maximum;
      shard_tile0        a carry: share of live rows that move at tile 0 of a later shard (the CARRY form of the move)."""
    live = moved = groups = mixed = carried = three = twice = late = s0 = 0
    faint = 1.0
    for prob in build(case, dtype):
        pl = plan(case, dtype, prob)
        mv, sees, s = pl["moves"], pl["sees"], pl["scores"]
        lv, m = sees.any(-1), mv.any(-1)
        live += int(lv.sum())
        moved += int(m.sum())
        late += int(mv.sum())
        carried += int((pl["share"][m] >= share_bar).sum())
        B, H, Sq, T = mv.shape
        pad = (-Sq) % 16
        mg = torch.nn.functional.pad(mv, (0, 0, 0, pad)).view(B, H, -1, 16, T)
        sg = torch.nn.functional.pad(sees, (0, 0, 0, pad)).view(B, H, -1, 16, T)
        mix = (mg.any(3) & (sg & ~mg).any(3)).any(-1)
        groups += mix.numel()
        mixed += int(mix.sum())
        r3 = sees.sum(-1) >= 3
        three += int(r3.sum())
        twice += int((r3 & (mv.sum(-1) >= 2)).sum())
        nvis = (~torch.isinf(s)).sum(-1)
        full = nvis >= 512
        if full.any():
            below = (s < s.amax(-1, keepdim=True) - 24.0).sum(-1)
            faint = min(faint, float((below[full].double() / nvis[full]).min()))
        if case.group == "carry":
            t0, at0 = 0, torch.zeros_like(lv)
            for lo, hi in shards(case, prob)[:-1]:
                t0 += (hi - lo + TILE - 1) // TILE
                at0 |= mv[..., t0]
            s0 += int(at0.sum())
    return {"live": live, "moved": moved / max(live, 1), "mixed": mixed / max(groups, 1), "carried": carried / max(moved, 1),
            "twice": twice / max(three, 1), "three": three, "late": late, "faint": faint, "shard_tile0": s0 / max(live, 1)}


# ---------------------------------------------------------------------------------------------------------------------
# reference and judgement
# ---------------------------------------------------------------------------------------------------------------------
def reference(prob, s=None):
    """fp64 (o [B,Sq,H,D], lse [B,H,Sq], natural units) of a problem: the softmax of its base-2 scores over prob.vv."""
    if s is None:
        s = scores_base2(prob.q, prob.kk, prob.c2)
        if prob.bias is not None:
            s = s + prob.bias
    H, Hkv = prob.q.shape[2], prob.vv.shape[2]
    m = s.amax(-1)
    empty = torch.isinf(m) & (m < 0)
    p = torch.exp2(s - torch.where(empty, torch.zeros_like(m), m)[..., None])
    p = torch.where(empty[..., None], torch.zeros_like(p), p)
    l = p.sum(-1)
    lse = torch.where(empty, m, (m + torch.log2(l)) * LN2)
    vd = prob.vv.double().repeat_interleave(H // Hkv, dim=2)
    o = torch.einsum("bhsk,bkhd->bshd", p / torch.where(empty, torch.ones_like(l), l)[..., None], vd)
    return o, lse


def lse_bar(dtype):
    """|lse - ref| absolute: every P is rounded with relative error <= u, so the row sum and with it lse are off by at
    most u; 2^-13 more for the fp32 steps and fp16's subnormal P.  4.0e-3 in bf16, 6.1e-4 in fp16."""
    return ac.U[dtype] + 2.0 ** -13


STATS: dict = {}   # (dtype, family) -> max of worst / mean / group (u) and lse (absolute) over the judge() calls of a process


def judge(o, lse, ref, ref_lse, dtype, family, what="", pl=None):
    """_attn_check.check of the output rows at the unchanged BARS[(dtype, family)] (its relative lse bar is not used), then
    the absolute lse bar.  A failure names the worst row and, given the plan (or a function that makes it), whether and
    where it moved."""
    def told(b, h, i):
        return describe_row(pl() if callable(pl) else pl, b, h, i) if pl is not None else f"row (b {b}, head {h}, query {i})"

    st = ac.measure(o, ref, dtype, None, ref_lse)
    live = ~(torch.isinf(ref_lse) & (ref_lse < 0))
    if lse is not None:
        dl = torch.where(live, (lse.double() - ref_lse).abs(), torch.zeros_like(ref_lse))
        st["lse"] = float(dl.nan_to_num(float("inf")).max()) if live.any() else 0.0
    rec = STATS.setdefault((dtype, family), {"worst": 0.0, "mean": 0.0, "group": 0.0, "lse": 0.0, "n": 0})
    for name in ("worst", "mean", "group", "lse"):
        if math.isfinite(st[name]):
            rec[name] = max(rec[name], st[name])
    rec["n"] += 1
    e = torch.where(live, ac.row_errors(o, ref), torch.zeros_like(ref_lse)).nan_to_num(float("inf"))
    b, h, i = (int(x) for x in torch.unravel_index(e.argmax(), e.shape))
    try:
        ac.check(o, ref, dtype, family, None, ref_lse, what)
    except AssertionError as err:
        raise AssertionError(f"{err}; worst {e[b, h, i] / ac.U[dtype]:.2f} u at {told(b, h, i)}") from None
    if lse is not None:
        assert torch.isfinite(lse[live]).all() and (lse[~live] == float("-inf")).all(), \
            f"{what}: lse not finite / not -inf where the reference's is"
        b, h, i = (int(x) for x in torch.unravel_index(dl.argmax(), dl.shape))
        assert st["lse"] <= lse_bar(dtype), (f"{what} [{family}]: |lse - ref| {st['lse']:.2e} (bar {lse_bar(dtype):.1e}) at "
                                            f"{told(b, h, i)}")
    return st


def chain(case, dtype, prob, defect=None):
    """lazy_chain over one problem the way the case launches it (a carry: shard by shard through an fp32 (o, lse) state).
    Returns (o fp32 [B,Sq,H,D], lse fp32)."""
    state = None
    for lo, hi in shards(case, prob):
        bias = None if prob.bias is None else prob.bias[..., lo:hi]
        state = lazy_chain(prob.q, prob.kk[:, lo:hi], prob.vv[:, lo:hi], prob.c2, dtype, case.rule, bias=bias, carried=state,
                           defect=defect)
    return state
