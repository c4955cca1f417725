"""Objective metrics of a rendered item against a target recording, on the GPU: the F0 frame error (FFE) with its voicing and gross-pitch parts,
the f0 RMSE in cents, a mel-cepstral distortion along a dynamic-time-warping path, and the cosine of the two speaker embeddings. The reference's
test step only pairs `mel_gt` with `mel_pred` and `f0_gt` with `f0_pred` and dumps them for offline scoring (tasks/StyleSinger/stylesinger.py:209-233);
here the score is computed in the process that rendered the item, with no host numpy between waveform and number: the mel front end, the f0
tracker, the speaker encoder and the resampler are the ones the input producers use, the metric stage is `csrc/evaluate.hip`.

NOT CLAIMED: this "MCD" is a LOG-MEL cepstral distortion of this project's own definition (the DCT-II of the clipped log10 mel the front end
writes). It is not the SPTK / WORLD mel-cepstrum MCD, parity with pymcd or any published tool is UNPINNED, and its absolute values are comparable
only with themselves (the same definition on both sides of a comparison). FFE follows the usual definition (voicing decision errors plus gross
pitch errors beyond 20 %, over all path cells), on this project's own f0 tracker.

Definitions (plain numpy / int on the host; the kernels are tested against them). Item a = the rendered side (rows i, n_a frames), item b = the
target (columns j, n_b frames), both on the mel hop grid.
  1. `mcep_q`: m = clip(mel, vmin, vmax) in fp32; tab[k][n] = fl32(sqrt(2 / N) cos(pi k (n + 0.5) / N)), k = 1 .. K (`mcep_table`, float64 rounded
     once); c_k = 0, then for n = 0 .. N - 1 IN THAT ORDER c_k = fl32(c_k + fl32(m[n] * tab[k][n])) - no fused multiply-add, so a numpy float32 loop
     restates the kernel bit for bit (a float64 evaluation of the sum differs in a few 1e-5 of the quantised values: the order is part of the
     definition); q_k = (int16) rint(fl32(c_k * s)), s = 256. Frames at or past n and the pad column (Kp = K rounded up to even) are 0.
     Range (`mcep_bound`): for K < N the rows are orthonormal, so |c_k| and ||c_a - c_b|| are at most sqrt(N) times the largest |m| / |m_a - m_b|:
     67.1 at N = 80 and [-6, 1.5], |q| <= 17174, S = sum_k (qa_k - qb_k)^2 <= 2.95e8 < 2^31. Settings whose bound leaves int16 are refused.
  2. `dtw_path`: cost c(i, j) = isqrt(S(i, j)) (the exact integer floor square root); band, centres c_i, W, the "not aligned" rule (n_b > W n_a or
     an empty item: status 1) and INF are those of `pitch.contour_align` (a = the score side, b = the guide side);
     D[i][j] = c + min over existing cells, the FIRST minimum in the order DIAGONAL, UP, LEFT. Not contour_align's order: with up first, two
     stretches of silence (identical clipped frames, zero costs) give a path that hugs the matrix edge and inflates the path length the means are
     taken over. -> the path in forward order, P, cost = D[n_a-1][n_b-1], status. With align="frames" or status 1 the path is the identity over
     min(n_a, n_b) frames (the reference's own truncation, :231-233).
  3. `path_metrics`: along the path, with f0 in Hz (0 = unvoiced): P, n_both (both voiced), n_vde (exactly one voiced), n_gpe (both voiced and
     fabsf(fa - fb) > 0.2f * fb in fp32), dist_sum = sum sqrt((double) S), cents_sq_sum = sum over both-voiced cells of (1200 log2(fa / fb))^2 in
     float64. `derive`: mcd_db = 10 sqrt(2) dist_sum / (s P), ffe = (n_vde + n_gpe) / P, vde = n_vde / P, gpe = n_gpe / max(n_both, 1),
     f0_rmse_cents = sqrt(cents_sq_sum / max(n_both, 1)).
  4. `singer_cos` = <ea, eb> / (|ea| |eb|) of the two speaker embeddings.

`python -m stylesinger_amd.evaluate --pred a.wav --target b.wav [--speaker-ckpt pretrained.pt] [--align dtw|frames] [--band-s 2.0] [--json out.json]`
scores two recordings (needs a GPU, no model checkpoint)."""
import json
import math
import warnings

import numpy as np
import torch

from . import lib as L

EVAL_K = 24                    # cepstral coefficients c1 .. c24 (c0, the frame's level, is left out)
EVAL_SCALE = 256.0             # q = rint(c * EVAL_SCALE): 1 / 256 of a log10 unit per count
EVAL_MAX_T = L.abi.DEFINES["SS_EVAL_MAX_T"]   # frames per item the aligner holds (its rolling diagonals live in LDS); refused beyond, never truncated
EVAL_MAX_K = L.abi.DEFINES["SS_EVAL_MAX_K"]
EVAL_INF = 0x3FFFFFFF          # D of a cell no path reaches (= pitch.ALIGN_INF)
EVAL_BAND_S = 2.0              # default half-width of the band, seconds around the linear fit
EVAL_MAX_WORKSPACE_BYTES = 4 << 30            # align_device refuses to allocate more cost + direction bytes than this for one call
GPE_REL = np.float32(0.2)      # gross pitch error: more than 20 % off the target


# ---- 1. quantised mel cepstrum ---------------------------------------------------------------------------------------------------------------------
def mcep_table(n_mels, K=EVAL_K):
    """tab [K][n_mels] fp32: row k - 1 = fl32(sqrt(2 / N) cos(pi k (n + 0.5) / N)), the orthonormal DCT-II without c0, computed in float64."""
    N = int(n_mels)
    k = np.arange(1, int(K) + 1, dtype=np.float64)[:, None]
    n = np.arange(N, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / N) * np.cos(np.pi * k * (n + 0.5) / N)).astype(np.float32)


def mcep_bound(n_mels, K, s, vmin, vmax):
    """The largest |q| and |qa - qb| a setting can produce (+ 1 for the rounding of the chain and of rint). K < N: Parseval on orthonormal rows;
    K >= N: rows repeat as aliases and one of them has norm sqrt(2). ValueError where int16 would not hold it, or (K >= N) int32 not hold S."""
    N, K = int(n_mels), int(K)
    if not (float(s) > 0 and float(vmin) < float(vmax)):
        raise ValueError(f"evaluate: scale {s} / range [{vmin}, {vmax}]")
    span = max(float(vmax) - float(vmin), abs(float(vmin)), abs(float(vmax)))
    bound = float(s) * math.sqrt(N) * span * (1.0 if K < N else math.sqrt(2.0)) + 1.0
    if bound > 32767.0 or (K >= N and K * bound * bound >= 2.0 ** 31):
        raise ValueError(f"evaluate: scale {s} over [{vmin}, {vmax}] at {N} bins, {K} coefficients reaches {bound:.0f}: beyond int16 "
                         "(refused, never truncated)")
    return bound


def mcep_q(mel, n=None, K=EVAL_K, s=EVAL_SCALE, vmin=-6.0, vmax=1.5):
    """mel [T, N] (log10, as the front end writes it), n valid frames (None: T) -> q int16 [T, Kp]: definition 1, the fp32 chain as a numpy loop."""
    mel = np.asarray(mel, dtype=np.float32)
    T, N = mel.shape
    n = T if n is None else min(int(n), T)
    mcep_bound(N, K, s, vmin, vmax)
    tab = mcep_table(N, K)
    Kp = (int(K) + 1) // 2 * 2
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.maximum(mel[:n], np.float32(vmin)), np.float32(vmax))
    c = np.zeros((n, int(K)), dtype=np.float32)
    for i in range(N):                                    # ascending n, every product and every sum rounded to fp32 on its own
        c = (c + (m[:, i, None] * tab[None, :, i]).astype(np.float32)).astype(np.float32)
    q = np.zeros((T, Kp), dtype=np.int16)
    q[:n, :int(K)] = np.rint((c * np.float32(s)).astype(np.float32)).astype(np.int16)
    return q


# ---- 2. alignment -------------------------------------------------------------------------------------------------------------------------------------
def sq_dist_matrix(qa, qb):
    """S(i, j) = sum_k (qa[i][k] - qb[j][k])^2 as int64 [n_a, n_b]."""
    qa, qb = np.asarray(qa, dtype=np.int64), np.asarray(qb, dtype=np.int64)
    S = np.zeros((qa.shape[0], qb.shape[0]), dtype=np.int64)
    for k in range(qa.shape[1]):
        d = qa[:, k, None] - qb[None, :, k]
        S += d * d
    return S


def isqrt(S):
    """floor(sqrt(S)) of non-negative int64 values, exact."""
    S = np.asarray(S, dtype=np.int64)
    r = np.floor(np.sqrt(S.astype(np.float64))).astype(np.int64)
    r -= (r * r > S)
    r += ((r + 1) * (r + 1) <= S)
    return r


def band_centres(n_a, n_b):
    """c_i = ((2 i + 1) n_b) // (2 n_a) (pitch.align_band_centres)."""
    i = np.arange(n_a, dtype=np.int64)
    return ((2 * i + 1) * n_b) // (2 * n_a)


def warp_path(C, W=None):
    """The warp of an integer cost matrix C [n_a, n_b] within the band |j - c_i| <= W (None: full): D[0][0] = C[0][0],
    D[i][j] = C[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors inside the band, the FIRST minimum in that order
    (diagonal, up, left); walked back from the far corner. -> (path int32 [P, 2] in forward order, cost) or (None, None) when the band does not
    connect the corners. A scalar loop on Python integers: this is the definition."""
    C = np.asarray(C)
    n_a, n_b = C.shape
    W = max(n_a, n_b) if W is None else int(W)
    ci = band_centres(n_a, n_b)
    lo, hi = np.maximum(ci - W, 0).tolist(), np.minimum(ci + W, n_b - 1).tolist()
    rows = C.tolist()
    INF = EVAL_INF
    D, step = [], []
    for i in range(n_a):
        l, h, c = lo[i], hi[i], rows[i]
        Di, Si = [INF] * (h - l + 1), [0] * (h - l + 1)
        if i > 0:
            pl, ph, Dp = lo[i - 1], hi[i - 1], D[i - 1]
        for j in range(l, h + 1):
            if i == 0 and j == 0:
                Di[0] = c[0]
                continue
            diag = Dp[j - 1 - pl] if i > 0 and pl <= j - 1 <= ph else INF
            up = Dp[j - pl] if i > 0 and pl <= j <= ph else INF
            left = Di[j - 1 - l] if j - 1 >= l else INF
            best, k = diag, 0                             # the first minimum: diagonal, up, left
            if up < best:
                best, k = up, 1
            if left < best:
                best, k = left, 2
            Si[j - l] = k
            Di[j - l] = INF if best >= INF else best + c[j]
        D.append(Di)
        step.append(Si)
    if lo[0] > 0 or hi[n_a - 1] < n_b - 1 or D[n_a - 1][n_b - 1 - lo[n_a - 1]] >= INF:
        return None, None
    path = []
    i, j = n_a - 1, n_b - 1
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        k = step[i][j - lo[i]]
        i, j = (i - 1, j - 1) if k == 0 else (i - 1, j) if k == 1 else (i, j - 1)
    return np.asarray(path[::-1], dtype=np.int32).reshape(-1, 2), int(D[n_a - 1][n_b - 1 - lo[n_a - 1]])


def identity_path(n_a, n_b):
    p = np.arange(min(int(n_a), int(n_b)), dtype=np.int32)
    return np.stack([p, p], axis=1).reshape(-1, 2)


def dtw_path(qa, qb, band=None):
    """Definition 2 for one item: qa int16 [n_a, Kp], qb int16 [n_b, Kp], band = half-width in frames of b (None or <= 0: full)
    -> (path int32 [P, 2], P, cost, status). status 1 (an empty item, or n_b > W n_a): the identity over min(n_a, n_b) frames, cost 0."""
    qa, qb = np.asarray(qa), np.asarray(qb)
    n_a, n_b = qa.shape[0], qb.shape[0]
    full = max(n_a, n_b)
    W = full if band is None or int(band) <= 0 or int(band) > full else int(band)
    if n_a == 0 or n_b == 0 or n_b > W * n_a:
        p = identity_path(n_a, n_b)
        return p, len(p), 0, 1
    path, cost = warp_path(isqrt(sq_dist_matrix(qa, qb)), W)
    assert path is not None, "a band with n_b <= W n_a is connected"
    return path, len(path), cost, 0


# ---- 3. metrics along the path -----------------------------------------------------------------------------------------------------------------------
def path_metrics(qa, qb, f0a, f0b, path):
    """Definition 3 for one item -> dict(P, n_both, n_vde, n_gpe (ints), dist_sum, cents_sq_sum (float64, math.fsum: the exact sum rounded once))."""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    P = len(path)
    if P == 0:
        return dict(P=0, n_both=0, n_vde=0, n_gpe=0, dist_sum=0.0, cents_sq_sum=0.0)
    i, j = path[:, 0], path[:, 1]
    d = np.asarray(qa, dtype=np.int64)[i] - np.asarray(qb, dtype=np.int64)[j]
    S = (d * d).sum(axis=1)
    fa, fb = np.asarray(f0a, dtype=np.float32)[i], np.asarray(f0b, dtype=np.float32)[j]
    va, vb = fa > 0, fb > 0
    both = va & vb
    gross = both & (np.abs(fa - fb) > GPE_REL * fb)       # fp32: the difference, the product and the comparison
    with np.errstate(divide="ignore", invalid="ignore"):
        cents = 1200.0 * np.log2(fa[both].astype(np.float64) / fb[both].astype(np.float64))
    return dict(P=P, n_both=int(both.sum()), n_vde=int((va != vb).sum()), n_gpe=int(gross.sum()),
                dist_sum=math.fsum(np.sqrt(S.astype(np.float64)).tolist()), cents_sq_sum=math.fsum((cents * cents).tolist()))


def derive(P, n_both, n_vde, n_gpe, dist_sum, cents_sq_sum, s=EVAL_SCALE):
    """The reported numbers of one item from its counts and sums (host arithmetic, float64). An item with P = 0 has no metrics: NaN."""
    if P <= 0:
        return dict(mcd_db=float("nan"), ffe=float("nan"), vde=float("nan"), gpe=float("nan"), f0_rmse_cents=float("nan"))
    nb = max(int(n_both), 1)
    return dict(mcd_db=10.0 * math.sqrt(2.0) * float(dist_sum) / (float(s) * P), ffe=(n_vde + n_gpe) / P, vde=n_vde / P, gpe=n_gpe / nb,
                f0_rmse_cents=math.sqrt(float(cents_sq_sum) / nb))


def singer_cos(ea, eb):
    """Definition 4 in float64; 0 where an embedding is all zero."""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    den = math.sqrt(float(ea @ ea)) * math.sqrt(float(eb @ eb))
    return float(ea @ eb) / den if den > 0 else 0.0


# ---- device forms --------------------------------------------------------------------------------------------------------------------------------------
def _need_device(what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise L.StyleSingerHipError(f"{what} needs device tensors: there is no CPU path")


def _lens(lens, B, width, dev):
    """Frame counts as an int32 device vector [B] (host ints, a tensor, or None = the buffer's width)."""
    t = torch.full((B,), int(width), dtype=torch.int32) if lens is None else torch.as_tensor(lens)
    t = t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if t.numel() != B:
        raise ValueError(f"evaluate: {t.numel()} lengths for {B} items")
    return t


_tab_cache = {}


def _table(n_mels, K, dev):
    key = (int(n_mels), int(K), str(dev))
    if key not in _tab_cache:
        _tab_cache[key] = torch.from_numpy(mcep_table(n_mels, K)).to(dev)
    return _tab_cache[key]


def _range(hparams):
    hp = hparams or {}
    return float(hp.get("mel_vmin", -6.0)), float(hp.get("mel_vmax", 1.5))


@torch.no_grad()
def mcep_q_device(mel, frames=None, hparams=None, K=EVAL_K):
    """mel fp32 [B, T, n_mels] on the device (log10, what `MelFrontendHIP.wav2mel` or the model writes), frames [B] valid frames (None: T) ->
    q int16 [B, T, Kp] (`ss_eval_mcep`): `mcep_q` of every item with hparams' mel_vmin / mel_vmax, zeros at and past frames[b]."""
    _need_device("mcep_q_device", mel)
    x = mel if mel.dtype == torch.float32 and mel.dim() == 3 and mel.stride(2) == 1 else mel.float().contiguous()
    if x.dim() != 3:
        raise ValueError(f"mcep_q_device: mel must be [B, T, n_mels] (got {tuple(mel.shape)})")
    B, T, N = x.shape
    vmin, vmax = _range(hparams)
    mcep_bound(N, K, EVAL_SCALE, vmin, vmax)
    if not 0 < int(K) <= EVAL_MAX_K:
        raise ValueError(f"mcep_q_device: K = {K} outside 1 .. {EVAL_MAX_K}")
    Kp = (int(K) + 1) // 2 * 2
    q = torch.empty(B, T, Kp, device=x.device, dtype=torch.int16)
    if B * T == 0:
        return q
    n = None if frames is None else _lens(frames, B, T, x.device)
    L.ops.ss_eval_mcep(x, x.stride(1), x.stride(0), n, _table(N, K, x.device), q, B, T, N, int(K), EVAL_SCALE, vmin, vmax)
    if n is not None:
        n.record_stream(torch.cuda.current_stream(x.device))
    return q


@torch.no_grad()
def align_device(qa, lens_a, qb, lens_b, band=None):
    """qa int16 [B, Ta, Kp], qb int16 [B, Tb, Kp] on the device, lens_a / lens_b [B] (host ints or device tensors; None = the widths), band =
    half-width in frames of b (None or <= 0: full) -> dict(path int32 [B, Ta + Tb, 2] (the first plen[b] pairs; the rest unspecified), plen, cost,
    status int32 [B], lens_a, lens_b (the int32 device vectors)): `dtw_path` of every item (`ss_eval_cost_band` + `ss_eval_dtw`). No host sync.
    Sizes beyond EVAL_MAX_T and a workspace above EVAL_MAX_WORKSPACE_BYTES are refused."""
    _need_device("align_device", qa, qb)
    if qa.dtype != torch.int16 or qb.dtype != torch.int16 or qa.dim() != 3 or qb.dim() != 3 or qa.shape[0] != qb.shape[0] or qa.shape[2] != qb.shape[2]:
        raise ValueError(f"align_device: qa {tuple(qa.shape)} {qa.dtype} / qb {tuple(qb.shape)} {qb.dtype}: int16 [B, T, Kp] with equal B and Kp")
    qa, qb = qa.contiguous(), qb.contiguous()
    B, Ta, Kp = qa.shape
    Tb = qb.shape[1]
    if Ta > EVAL_MAX_T or Tb > EVAL_MAX_T:
        raise ValueError(f"align_device: {Ta} / {Tb} frames exceed the aligner's cap of {EVAL_MAX_T}; score shorter items or use align='frames'")
    dev = qa.device
    la, lb = _lens(lens_a, B, Ta, dev), _lens(lens_b, B, Tb, dev)
    band = 0 if band is None or int(band) <= 0 else int(band)
    lib = L.load()
    ws_bytes = int(lib.ss_eval_dtw_workspace_bytes(B, Ta, Tb, band))
    if ws_bytes <= 0:
        raise L.StyleSingerHipError(f"ss_eval_dtw_workspace_bytes refused B={B} Ta={Ta} Tb={Tb} band={band}")
    if ws_bytes > EVAL_MAX_WORKSPACE_BYTES:
        raise ValueError(f"align_device: {ws_bytes} bytes of workspace for B={B} Ta={Ta} Tb={Tb} band={band or 'full'} exceed "
                         f"EVAL_MAX_WORKSPACE_BYTES = {EVAL_MAX_WORKSPACE_BYTES}; narrow the band or split the batch")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    path = torch.empty(B, Ta + Tb, 2, device=dev, dtype=torch.int32)
    plen, cost, status = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    L.ops.ss_eval_cost_band(qa, la, qb, lb, Kp, band, Ta, Tb, B, ws, ws_bytes)
    L.ops.ss_eval_dtw(la, lb, band, path, plen, cost, status, Ta, Tb, B, ws, ws_bytes)
    ws.record_stream(torch.cuda.current_stream(dev))
    return dict(path=path, plen=plen, cost=cost, status=status, lens_a=la, lens_b=lb)


@torch.no_grad()
def reduce_device(qa, f0_a, lens_a, qb, f0_b, lens_b, path=None, plen=None):
    """`path_metrics` of every item on the device (`ss_eval_reduce`): f0_a fp32 [B, >= Ta], f0_b fp32 [B, >= Tb] in Hz; path / plen as `align_device`
    returns them, or both None: the identity over min(n_a, n_b) frames -> (counts int64 [B, 4] = P, n_both, n_vde, n_gpe; sums float64 [B, 2] =
    dist_sum, cents_sq_sum). No host sync."""
    _need_device("reduce_device", qa, qb, f0_a, f0_b)
    qa, qb = qa.contiguous(), qb.contiguous()
    B, Ta, Kp = qa.shape
    Tb = qb.shape[1]
    dev = qa.device
    fa = f0_a if f0_a.dtype == torch.float32 and f0_a.stride(1) == 1 else f0_a.float().contiguous()
    fb = f0_b if f0_b.dtype == torch.float32 and f0_b.stride(1) == 1 else f0_b.float().contiguous()
    if fa.shape[0] != B or fb.shape[0] != B or fa.shape[1] < Ta or fb.shape[1] < Tb:
        raise ValueError(f"reduce_device: f0 {tuple(fa.shape)} / {tuple(fb.shape)} for q {tuple(qa.shape)} / {tuple(qb.shape)}")
    la, lb = _lens(lens_a, B, Ta, dev), _lens(lens_b, B, Tb, dev)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int64)
    sums = torch.empty(B, 2, device=dev, dtype=torch.float64)
    L.ops.ss_eval_reduce(qa, fa, fa.stride(0), la, qb, fb, fb.stride(0), lb, Kp, path, plen, Ta, Tb, B, counts, sums)
    for t in (la, lb):
        t.record_stream(torch.cuda.current_stream(dev))
    return counts, sums


@torch.no_grad()
def cosine_rows_device(a, b):
    """a, b fp32 [rows, C] on the device -> fp32 [rows]: the cosine of every row pair, sums in float64 (`ss_cosine_rows`)."""
    _need_device("cosine_rows_device", a, b)
    a, b = a.float().contiguous(), b.float().contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"cosine_rows_device: {tuple(a.shape)} against {tuple(b.shape)}")
    out = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
    L.ops.ss_cosine_rows(a, b, out, a.shape[0], a.shape[1])
    return out


def band_frames(band_s, sr, hop):
    """The band in frames: round(band_s * sr / hop); 0 = the full matrix. ValueError for a negative or non-finite time."""
    band_s = float(band_s)
    if not (band_s >= 0 and math.isfinite(band_s)):
        raise ValueError(f"evaluate: band_s = {band_s}: seconds >= 0 (0 = the full matrix)")
    return int(round(band_s * float(sr) / float(hop)))


DERIVED = ("mcd_db", "ffe", "vde", "gpe", "f0_rmse_cents")


@torch.no_grad()
def score_pairs(mel_a, f0_a, n_a, mel_b, f0_b, n_b, align="dtw", band_s=EVAL_BAND_S, hparams=None):
    """Score a batch of rendered items against their targets: mel_a [B, Ta, n_mels] / f0_a [B, >= Ta] (Hz, 0 = unvoiced) / n_a [B] frames = the
    rendered side, mel_b / f0_b / n_b the target, everything on the device and on the mel hop grid. align = "dtw" (the warp in a band of `band_s`
    seconds around the linear fit; 0 = the full matrix) or "frames" (frame p against frame p over min(n_a, n_b) frames, as the reference pairs them).
    -> dict with per-item DEVICE tensors counts [B, 4], sums [B, 2], cost, status, plen [B] (+ path for "dtw"), and - after ONE host sync at the
    end - the derived floats per item as float64 arrays (mcd_db, ffe, vde, gpe, f0_rmse_cents; NaN for an item without frames) and `mean`, their
    batch means over the items that have frames. Items the aligner did not align (status 1: scored on the identity path) are named in one warning.

    A style sweep is scored through its `emit` callback, no extra parameter:
        scores = []
        def emit(res):                                   # res = what infer_batch returns for one batch of the sweep
            scores.append(infer.evaluate(res, target_wavs, target_lens))        # or score_pairs(res["mel"], res["f0"], res["lens"], mel_b, f0_b, n_b)
        sweep.style_transfer_sweep(infer, ..., emit=emit)"""
    from .config import make_hparams
    hp = make_hparams(hparams)
    if align not in ("dtw", "frames"):
        raise ValueError(f"score_pairs: align = {align!r}: 'dtw' or 'frames'")
    band = band_frames(band_s, hp["audio_sample_rate"], hp["hop_size"])
    _need_device("score_pairs", mel_a, mel_b, f0_a, f0_b)
    qa = mcep_q_device(mel_a, n_a, hp)
    qb = mcep_q_device(mel_b, n_b, hp)
    B = qa.shape[0]
    out = {}
    if align == "dtw":
        al = align_device(qa, n_a, qb, n_b, band)
        counts, sums = reduce_device(qa, f0_a, al["lens_a"], qb, f0_b, al["lens_b"], al["path"], al["plen"])
        out.update(path=al["path"], plen=al["plen"], cost=al["cost"], status=al["status"])
    else:
        counts, sums = reduce_device(qa, f0_a, n_a, qb, f0_b, n_b)
        out.update(plen=counts[:, 0].to(torch.int32), cost=torch.zeros(B, device=qa.device, dtype=torch.int32),
                   status=torch.zeros(B, device=qa.device, dtype=torch.int32))
    out.update(counts=counts, sums=sums, align=align, band=band)
    host = torch.cat([counts.double(), sums, out["status"].double()[:, None]], dim=1).cpu().numpy()   # the one host sync
    per = [derive(int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4], r[5]) for r in host]
    for k in DERIVED:
        out[k] = np.asarray([p[k] for p in per], dtype=np.float64)
    have = host[:, 0] > 0
    out["mean"] = {k: float(out[k][have].mean()) if have.any() else float("nan") for k in DERIVED}
    bad = [i for i, v in enumerate(host[:, 6]) if v != 0]
    if bad:
        warnings.warn(f"evaluate: items {bad} not aligned (more target frames per rendered frame than the band allows, or empty): they were scored "
                      "frame against frame; widen band_s")
    return out


def _zero_padded(wav, lens, frames, hop):
    """wav [B, L] with lens valid samples -> [B, max(frames) * hop] fp32, exact zeros past every item's own samples (whatever the buffer held)."""
    B, Lw = wav.shape
    width = max(1, max(frames) * hop)
    n = torch.tensor([int(v) for v in lens], device=wav.device)[:, None]
    buf = torch.zeros(B, max(width, Lw), device=wav.device, dtype=torch.float32)
    buf[:, :Lw] = torch.where(torch.arange(Lw, device=wav.device)[None, :] < n, wav.float(), torch.zeros((), device=wav.device))
    return buf[:, :width].contiguous()


@torch.no_grad()
def score_wavs(infer_or_frontend, wav_a, lens_a, wav_b, lens_b, srs_b=None, align="dtw", band_s=EVAL_BAND_S, hparams=None):
    """Score rendered waveforms wav_a [B, La] (lens_a valid samples, host ints; at the model's sample rate) against target recordings wav_b [B, Lb]
    (lens_b; at the model's rate, or at the per-item rates `srs_b`: those items are resampled on the device first, the path of the reference
    audio). `infer_or_frontend`: a StyleSingerInfer (its mel front end; `singer_cos` is added when it has a speaker encoder) or a MelFrontendHIP.
    BOTH sides go through the same analysis - `wav2mel` and `track_f0_device` (80-800 Hz) on the audio zero-padded to its frame count - so the
    comparison is symmetric: an item against itself scores 0. Then `score_pairs`. -> its dict, + `singer_cos` (fp32 [B] on the device, and the
    batch mean in `mean`) and `frames_a`, `frames_b` (host ints)."""
    from .f0track import track_f0_device
    from .resample import resample_batch
    inf = infer_or_frontend if hasattr(infer_or_frontend, "_mel_front") else None
    front = inf._mel_front() if inf is not None else infer_or_frontend
    hp = dict(hparams or (inf.hparams if inf is not None else {}))
    sr, hop = int(front.sr), int(front.hop)
    hp.update(audio_sample_rate=sr, hop_size=hop)
    dev = front.device
    sides = []
    for wav, lens, srs in ((wav_a, lens_a, None), (wav_b, lens_b, srs_b)):
        wav = wav.to(dev).float()
        if wav.dim() == 1:
            wav = wav[None]
        lens = [int(v) for v in lens]
        if len(lens) != wav.shape[0]:
            raise ValueError(f"score_wavs: {len(lens)} lengths for {wav.shape[0]} waveforms")
        if srs is not None and any(int(r) != sr for r in srs):
            if len(srs) != len(lens):
                raise ValueError(f"score_wavs: {len(srs)} sample rates for {len(lens)} targets")
            rows = []
            for b, r in enumerate(srs):                  # (one launch per item of another rate; the grouped form is ReferenceProducers._resample_refs)
                y, (n,) = resample_batch(wav[b:b + 1, :max(1, lens[b])], [lens[b]], int(r), sr)
                rows.append((y[0, :n], n))
            lens = [n for _, n in rows]
            wav = torch.zeros(len(rows), max(1, max(lens)), device=dev, dtype=torch.float32)
            for b, (y, n) in enumerate(rows):
                wav[b, :n] = y
        frames = [n // hop + 1 for n in lens]            # frames of a centred STFT
        padded = _zero_padded(wav, lens, frames, hop)
        mel, fr = front.wav2mel(padded[:, :max(1, max(lens))], torch.tensor(lens, dtype=torch.int64))
        f0 = track_f0_device(padded, [f * hop for f in frames], mel.shape[1], sr=sr, hop_size=hop)
        sides.append(dict(mel=mel, f0=f0, frames=frames, n=fr, padded=padded))
    a, b = sides
    if len(a["frames"]) != len(b["frames"]):
        raise ValueError(f"score_wavs: {len(a['frames'])} rendered items against {len(b['frames'])} targets")
    out = score_pairs(a["mel"], a["f0"], a["n"], b["mel"], b["f0"], b["n"], align=align, band_s=band_s, hparams=hp)
    out.update(frames_a=a["frames"], frames_b=b["frames"])
    if inf is not None and getattr(inf, "speaker_encoder", None) is not None:
        ea = inf.embed_speaker_batch(a["padded"], [f * hop for f in a["frames"]])
        eb = inf.embed_speaker_batch(b["padded"], [f * hop for f in b["frames"]])
        out["singer_cos"] = cosine_rows_device(ea, eb)
        out["mean"]["singer_cos"] = float(out["singer_cos"].double().mean().item())
    return out


class _Scorer:
    """What the command line hands `score_wavs` in place of a StyleSingerInfer: the mel front end and, with --speaker-ckpt, the speaker encoder with
    the producers' own `embed_speaker_batch` (no model, no vocoder)."""

    def __init__(self, hparams=None, speaker_state=None, device="cuda"):
        from .config import make_hparams
        from .producers import ReferenceProducers
        self.hparams = make_hparams(hparams)
        self._front_hparams = hparams
        self.device = torch.device(device)
        self._mel_frontend = self._emo_frontend = None
        self.speaker_encoder = None
        if speaker_state is not None:
            from .speaker import SpeakerEncoderHIP
            self.speaker_encoder = SpeakerEncoderHIP(speaker_state, device=self.device)
        for name in ("_mel_front", "_emo_front", "_partials_batch", "_mean_l2norm_per_item", "embed_speaker_batch"):
            setattr(self, name, getattr(ReferenceProducers, name).__get__(self))


def main(argv=None):
    """`python -m stylesinger_amd.evaluate --pred a.wav --target b.wav [--speaker-ckpt pretrained.pt] [--align dtw|frames] [--band-s 2.0]
    [--json out.json]`: score one rendered recording against one target (WAV files of any rate: both are resampled to the model's rate on the
    device). Prints the numbers as one JSON object; `--json` also writes them to a file. Needs a GPU, no model checkpoint."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylesinger_amd.evaluate",
                                 description="FFE, f0 RMSE, log-mel cepstral distortion along a DTW path and singer cosine of two recordings, on the GPU "
                                             "(this project's own definitions: not SPTK / WORLD MCD)")
    ap.add_argument("--pred", required=True, help="the rendered recording (WAV)")
    ap.add_argument("--target", required=True, help="the target recording (WAV)")
    ap.add_argument("--speaker-ckpt", help="resemblyzer's pretrained.pt: adds singer_cos")
    ap.add_argument("--align", choices=["dtw", "frames"], default=None, help="dtw (default): warp the target onto the rendering; frames: frame against frame")
    ap.add_argument("--band-s", type=float, help=f"--align dtw: half-width of the band around the linear fit, seconds (default {EVAL_BAND_S}; 0 = full)")
    ap.add_argument("--json", help="also write the result to this file")
    a = ap.parse_args(argv)
    if a.band_s is not None and a.align != "dtw":
        ap.error("--band-s needs --align dtw")
    if a.band_s is not None and not (a.band_s >= 0 and math.isfinite(a.band_s)):
        ap.error("--band-s: seconds >= 0 (0 = full)")
    from .audiofile import load_audio
    from .resample import resample_batch
    if not torch.cuda.is_available():
        raise L.StyleSingerHipError("python -m stylesinger_amd.evaluate needs a GPU: there is no CPU path")
    spk = None
    if a.speaker_ckpt:
        spk = torch.load(a.speaker_ckpt, map_location="cpu", weights_only=False)
        spk = spk.get("model_state", spk)
    sc = _Scorer(None, speaker_state=spk)
    sr = int(sc.hparams["audio_sample_rate"])
    pred, sr_p = load_audio(a.pred)
    tgt, sr_t = load_audio(a.target)
    wa = torch.from_numpy(np.ascontiguousarray(pred))[None].to(sc.device)
    wa, (na,) = resample_batch(wa, [len(pred)], sr_p, sr)
    wb = torch.from_numpy(np.ascontiguousarray(tgt))[None].to(sc.device)
    res = score_wavs(sc, wa, [na], wb, [len(tgt)], srs_b=[sr_t], align=a.align or "dtw", band_s=EVAL_BAND_S if a.band_s is None else a.band_s)
    rep = dict(pred=a.pred, target=a.target, align=res["align"], band_frames=res["band"], frames_pred=res["frames_a"][0], frames_target=res["frames_b"][0],
               path_len=int(res["plen"][0].item()), status=int(res["status"][0].item()), cost=int(res["cost"][0].item()),
               **{k: float(res[k][0]) for k in DERIVED})
    if "singer_cos" in res:
        rep["singer_cos"] = float(res["singer_cos"][0].item())
    rep["note"] = "mcd_db is a log-mel cepstral distortion of this project's own definition, not SPTK / WORLD MCD"
    text = json.dumps(rep, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(text + "\n")
    return rep


if __name__ == "__main__":
    main()
