"""Reference-f0 conditioning: mirror of `utils/pitch_utils.py:34-62` (`norm_f0`, `norm_interp_f0`).

`inference/StyleSinger.py:152` feeds the tracker's contour (Hz, 0 = unvoiced) through `norm_interp_f0` before the model sees
it: log2(f0 + 1e-8) (`pitch_norm: log`), unvoiced frames replaced by a linear interpolation between their voiced neighbours
(`np.interp`: held flat beyond the first / last voiced frame), all-unvoiced contours become 0.

Two forms with the same contract:
  * `norm_interp_f0(f0, hparams)`      host numpy, what `StyleSingerInfer.input_to_batch` calls for one utterance;
  * `norm_interp_f0_device(f0, lens)`  `[B, T]` on the GPU (`ss_norm_interp_f0`), what `preprocess_batch` uses so a batch
                                       goes from tracker output to `infer_batch` without a host round trip.

Pitch control (`StyleSingerHIP.forward(pitch_hz=...)`): a caller's contour in Hz lives on a frame grid of its own, the score's frame count is only
known inside forward. `contour_fit` is the float64 definition of the fit between the two grids, `contour_fit_device` the kernel (`ss_contour_fit`,
csrc/pitch_fit.hip) that runs it from device lengths. That fit is a linear time scaling: right for a contour that already has the score's timing.
A guide vocal does not: `contour_align` (definition, integer arithmetic) / `contour_align_device` (`ss_contour_align`, csrc/contour_align.hip) warp
the contour onto the score's per-frame notes by dynamic time warping (forward(pitch_align="dtw")). The reverse direction - the score laid out on the
GUIDE's frames, so that the render is in sync with the take - is `retime_to_guide` (definition, integers only) / `retime_device` (`ss_retime_mel2ph`,
csrc/retime.hip): the alignment's path turned into a new mel2ph of the guide's length (forward(pitch_timing="guide")).

Pitch expression controls (forward(pitch_correct=, vibrato_scale=, vibrato_add=, pitch_smooth_ms=)): an edit of the merged log2-f0 of ANY branch,
predicted or given, between the pitch tail and pitch_embed. `pitch_edit` is the float64 definition (a Hann moving average splits the contour into a
trend and what rides on it; the trend is pulled toward the score's notes, the rest scaled, a synthetic vibrato added to held notes),
`pitch_edit_device` the kernels (`ss_pitch_edit_runs`, `ss_pitch_edit`, csrc/pitch_edit.hip), `controls.resolve_pitch_edit` the argument rules every
entry point shares.
"""
import numpy as np
import torch

from . import lib as L
from .controls import EDIT_SMOOTH_MS, edit_window_frames, resolve_pitch_edit  # noqa: F401  (the edit's window and argument rules: part of this module's surface)


def norm_f0(f0, uv, hparams):
    """utils/pitch_utils.py:34-45 for numpy input. Returns a new array."""
    f0 = np.array(f0, copy=True)
    if hparams.get("pitch_norm", "log") == "standard":
        f0 = (f0 - hparams.get("f0_mean", 400)) / hparams.get("f0_std", 100)
    if hparams.get("pitch_norm", "log") == "log":
        f0 = np.log2(f0 + 1e-8)
    if uv is not None and hparams.get("use_uv", True):
        f0[uv > 0] = 0
    return f0


def norm_interp_f0(f0, hparams):
    """utils/pitch_utils.py:47-62: f0 [T] in Hz (numpy or torch, any float dtype; the arithmetic runs in the input's dtype
    as numpy does there) -> (f0 [T] float32 tensor, uv [T] float32 tensor)."""
    is_torch = isinstance(f0, torch.Tensor)
    device = f0.device if is_torch else None
    x = f0.detach().cpu().numpy() if is_torch else np.asarray(f0)
    uv = x == 0
    y = norm_f0(x, uv, hparams)
    n_uv = int(uv.sum())
    if n_uv == len(y):
        y[uv] = 0
    elif n_uv > 0:
        y[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], y[~uv])
    f0_t = torch.from_numpy(np.asarray(y, dtype=np.float32))
    uv_t = torch.from_numpy(uv.astype(np.float32))
    if is_torch:
        f0_t, uv_t = f0_t.to(device), uv_t.to(device)
    return f0_t, uv_t


@torch.no_grad()
def norm_interp_f0_device(f0_hz, lens=None, hparams=None):
    """f0_hz fp32 [B, T] on the device (0 = unvoiced), lens int32 [B] valid frames per item (default T) ->
    (f0 [B, T], uv [B, T]) fp32: per item `norm_interp_f0` of its first lens[b] frames; frames >= lens[b] are 0. Contract: the entry takes
    FP32 Hz, i.e. what numpy computes on a float32 contour (log2 and the interpolation weights in double, the interpolation endpoints rounded to
    fp32 first); against the reference's float64 tracker output that is within 1 fp32 ulp of values in [6, 10] (tests allow 2e-6), not
    bit-identical to the host path `norm_interp_f0` of this module, which `input_to_batch` uses on the float64 contour."""
    hp = hparams or {}
    if hp.get("pitch_norm", "log") != "log" or not hp.get("use_uv", True):
        raise NotImplementedError("norm_interp_f0_device: only pitch_norm='log' with use_uv (the reference's setting)")
    if f0_hz.device.type != "cuda":
        raise L.StyleSingerHipError("norm_interp_f0_device needs device tensors: there is no CPU path")
    x = f0_hz.float().contiguous()
    B, T = x.shape
    out = torch.empty_like(x)
    uv = torch.empty_like(x)
    lp = None if lens is None else lens.to(device=x.device, dtype=torch.int32).contiguous()
    L.ops.ss_norm_interp_f0(x, lp, out, uv, B, T)
    return out, uv


def contour_fit(f0_hz, n_t, shift=0.0):
    """The definition of the contour fit (float64): f0_hz [n_c] in Hz (0 = unvoiced) -> [n_t] in Hz on a grid of n_t frames over the same time span.
    Output frame t sits at source position s = (t + 0.5) * n_c / n_t - 0.5, clamped to [0, n_c - 1] (the frame centres of both grids on one time
    axis); s is held as the exact fraction num / (2 n_t). With i0 = floor(s), fr = s - i0, i1 = min(i0 + 1, n_c - 1):
      * the frame is voiced iff the NEAREST source frame is voiced (fr >= 1/2 -> i1: a tie goes to the later frame), else 0;
      * its value is exp2((1 - fr) log2 f[i0] + fr log2 f[i1]) when both neighbours are voiced, otherwise the nearest frame's value (then the only
        voiced neighbour), times 2^(shift / 12) (shift in semitones);
      * fr == 0 takes f[i0] itself, so with shift == 0 equal lengths return the contour unchanged, bit for bit."""
    f = np.asarray(f0_hz, dtype=np.float64)
    n_c, n_t = len(f), int(n_t)
    out = np.zeros(n_t, dtype=np.float64)
    if n_c == 0 or n_t == 0:
        return out
    t = np.arange(n_t, dtype=np.int64)
    den = 2 * n_t
    num = np.clip((2 * t + 1) * n_c - n_t, 0, (n_c - 1) * den)
    i0, rem = num // den, num % den
    i1 = np.minimum(i0 + 1, n_c - 1)
    a, c = f[i0], f[i1]
    near = np.where(2 * rem >= den, c, a)
    fr = rem / den
    both = (a > 0) & (c > 0) & (rem != 0)
    with np.errstate(divide="ignore"):
        la, lc = np.log2(np.where(both, a, 1.0)), np.log2(np.where(both, c, 1.0))
    val = np.where(both, np.exp2(la + fr * (lc - la)), near)
    voiced = near > 0
    out[voiced] = val[voiced] * (2.0 ** (float(shift) / 12.0) if shift else 1.0)
    return out


@torch.no_grad()
def contour_fit_device(f0_hz, lens_c, lens_t, T, shift=0.0):
    """f0_hz fp32 [B, Lc] on the device (Hz, 0 = unvoiced), lens_c [B] valid source frames (host ints or a device tensor; None = Lc), lens_t int32 [B] ON THE
    DEVICE (target frames per item: no host sync) -> [B, T] fp32: `contour_fit` of each item's first lens_c[b] frames to lens_t[b] frames, 0 beyond."""
    if not torch.is_tensor(f0_hz) or f0_hz.device.type != "cuda":
        raise L.StyleSingerHipError("contour_fit_device needs device tensors: there is no CPU path")
    x = f0_hz if f0_hz.dtype == torch.float32 and f0_hz.stride(1) == 1 and f0_hz.stride(0) >= f0_hz.shape[1] else f0_hz.float().contiguous()
    B, Lc = x.shape
    dev = x.device
    lc = torch.full((B,), Lc, dtype=torch.int32) if lens_c is None else torch.as_tensor(lens_c)
    lc = lc.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    lt = lens_t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if lc.numel() != B or lt.numel() != B:
        raise ValueError(f"contour_fit_device: {lc.numel()} source lengths and {lt.numel()} target lengths for {B} contours")
    out = torch.empty(B, int(T), device=dev, dtype=torch.float32)
    L.ops.ss_contour_fit(x, x.stride(0), Lc, lc, lt, float(shift), out, out.stride(0), int(T), B)
    return out


# ---- contour alignment by dynamic time warping (forward(pitch_align="dtw")) ----------------------------------------------------------------------
# Named here, passed to the kernel as arguments, not user options.
ALIGN_CAP = 1200        # cents: a voiced pair further apart than an octave costs the same, everything beyond is equally wrong
ALIGN_UV_COST = 300     # cents: a voicing mismatch costs what leaving the model's +-3 semitone window around the note costs (ss_f0_bounds)
ALIGN_UNVOICED = -32768                    # the cents arrays' sentinel (int16) for an unvoiced guide frame / a rest
ALIGN_CENTS_LO, ALIGN_CENTS_HI = -2000, 16000   # guide cents are clipped to this range and notes to MIDI 1..127 (100 .. 12700 cents): both ends lie
#                                                 more than ALIGN_CAP outside the notes' range, so the clip cannot change a cost
ALIGN_INF = 0x3FFFFFFF                     # D of a cell no path reaches
ALIGN_MAX_T = L.ALIGN_MAX_T       # the kernel's caps (the LDS its layout needs): sizes beyond them are refused, never truncated
ALIGN_MAX_LC = L.ALIGN_MAX_LC
ALIGN_MAX_WORKSPACE_BYTES = 4 << 30        # contour_align_device refuses to allocate more direction bytes than this for one call


def align_cents(f0_hz, shift=0.0):
    """Guide frames in integer cents as the kernel computes them (fp32): 6900 + lrintf(1200 log2f(g / 440) + 100 shift) with every product and the
    sum rounded to fp32 on its own, clipped to [ALIGN_CENTS_LO, ALIGN_CENTS_HI]; ALIGN_UNVOICED where not g > 0."""
    g = np.asarray(f0_hz, dtype=np.float32)
    v = g > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.float32(1200.0) * np.log2(np.where(v, g, np.float32(440.0)) / np.float32(440.0), dtype=np.float32) + np.float32(100.0) * np.float32(shift)
    x = np.clip(x.astype(np.float32), np.float32(ALIGN_CENTS_LO - 6900), np.float32(ALIGN_CENTS_HI - 6900))
    return np.where(v, 6900 + np.rint(x).astype(np.int64), ALIGN_UNVOICED).astype(np.int64)


def align_cost_matrix(Gc, Mc, uv_cost=ALIGN_UV_COST, cap=ALIGN_CAP):
    """c(i, j) int64 [n_t, n_c] of score cents Mc [n_t] and guide cents Gc [n_c] (ALIGN_UNVOICED = unvoiced / rest)."""
    Gc, Mc = np.asarray(Gc, dtype=np.int64)[None, :], np.asarray(Mc, dtype=np.int64)[:, None]
    gv, mv = Gc != ALIGN_UNVOICED, Mc != ALIGN_UNVOICED
    return np.where(gv & mv, np.minimum(np.abs(Gc - Mc), cap), np.where(gv != mv, uv_cost, 0)).astype(np.int64)


def align_band_centres(n_t, n_c):
    """c_i = ((2 i + 1) n_c) // (2 n_t): the guide frame under the centre of score frame i (the frame-centre rule of contour_fit, exact integers)."""
    i = np.arange(n_t, dtype=np.int64)
    return ((2 * i + 1) * n_c) // (2 * n_t)


def align_path(C, W=None):
    """The warp of a cost matrix C [n_t, n_c] (n_t, n_c >= 1; integers) within the band |j - c_i| <= W (None: full, W = max(n_t, n_c)):
    D[0][0] = C[0][0], D[i][j] = C[i][j] + min(D[i-1][j], D[i][j-1], D[i-1][j-1]) over the predecessors inside the band, the FIRST minimum in that
    order (up, left, diagonal); walk back from (n_t-1, n_c-1) to (0, 0); idx[i] = the smallest j the path visits in row i.
    -> (idx int64 [n_t], cost) or (None, None) when the end cell cannot be reached from (0, 0) inside the band."""
    C = np.asarray(C)
    n_t, n_c = C.shape
    W = max(n_t, n_c) if W is None else int(W)
    ci = align_band_centres(n_t, n_c)
    lo, hi = np.maximum(ci - W, 0).tolist(), np.minimum(ci + W, n_c - 1).tolist()
    rows = C.tolist()                                   # plain Python integers: the loop below is the definition, kept scalar
    INF = ALIGN_INF
    D, step = [], []                                    # per row: the cells lo[i] .. hi[i]
    for i in range(n_t):
        l, h, c = lo[i], hi[i], rows[i]
        Di, Si = [INF] * (h - l + 1), [0] * (h - l + 1)
        if i > 0:
            pl, ph, Dp = lo[i - 1], hi[i - 1], D[i - 1]
        for j in range(l, h + 1):
            if i == 0 and j == 0:
                Di[0] = c[0]
                continue
            up = Dp[j - pl] if i > 0 and pl <= j <= ph else INF
            left = Di[j - 1 - l] if j - 1 >= l else INF
            diag = Dp[j - 1 - pl] if i > 0 and pl <= j - 1 <= ph else INF
            best, k = up, 0                             # the first minimum: up, left, diagonal
            if left < best:
                best, k = left, 1
            if diag < best:
                best, k = diag, 2
            Si[j - l] = k
            Di[j - l] = INF if best >= INF else best + c[j]
        D.append(Di)
        step.append(Si)
    if lo[0] > 0 or hi[n_t - 1] < n_c - 1 or D[n_t - 1][n_c - 1 - lo[n_t - 1]] >= INF:
        return None, None
    idx = np.zeros(n_t, dtype=np.int64)
    i, j = n_t - 1, n_c - 1
    while True:
        idx[i] = j   # j only falls along the walk: the last write of a row is its smallest j
        if i == 0 and j == 0:
            break
        k = step[i][j - lo[i]]
        i, j = (i - 1, j) if k == 0 else (i, j - 1) if k == 1 else (i - 1, j - 1)
    return idx, int(D[n_t - 1][n_c - 1 - lo[n_t - 1]])


def contour_align(f0_hz, midi, band=None, shift=0.0, uv_cost=ALIGN_UV_COST, cap=ALIGN_CAP):
    """The definition of the contour alignment (one item): guide f0_hz [n_c] in Hz (0 = unvoiced) warped onto the score's per-frame notes
    midi [n_t] (MIDI numbers, <= 0 = rest; what ss_gather_expand_i64(note, mel2ph) gives) by dynamic time warping.
      * cents: guide `align_cents(f0_hz, shift)` (the SHIFTED guide is compared: pitch_shift is how the caller puts the guide into the score's key);
        score 100 * min(m, 127);
      * cost c(i, j): both voiced min(|Gc[j] - Mc[i]|, cap); exactly one voiced uv_cost; neither 0;
      * band: cell (i, j) exists iff |j - c_i| <= W, c_i = ((2 i + 1) n_c) // (2 n_t); band None or <= 0: full, W = max(n_t, n_c);
      * recurrence, tie order and result: `align_path`; out[i] = fl32(fl32(g[idx[i]]) * fl32(2^(shift / 12))), 0 where g[idx[i]] is unvoiced.
    An item with n_c > W n_t (more than W guide frames per score frame: the band would be disconnected) is NOT aligned: status 1, out =
    contour_fit(f0_hz, n_t, shift) (its float64 definition; the kernel runs the arithmetic of ss_contour_fit), idx = -1, cost = 0. Empty items
    (n_t == 0 or n_c == 0): status 1, zeros.
    -> (out [n_t] (fp32 when aligned), idx int32 [n_t], cost int, status int)."""
    g = np.asarray(f0_hz, dtype=np.float32)
    m = np.asarray(midi, dtype=np.int64)
    n_c, n_t = len(g), len(m)
    W = max(n_t, n_c) if band is None or int(band) <= 0 else int(band)
    if n_t == 0 or n_c == 0:
        return np.zeros(n_t, dtype=np.float32), np.full(n_t, -1, dtype=np.int32), 0, 1
    if n_c > W * n_t:
        return contour_fit(g, n_t, shift), np.full(n_t, -1, dtype=np.int32), 0, 1
    Mc = np.where(m > 0, 100 * np.minimum(m, 127), ALIGN_UNVOICED)
    idx, cost = align_path(align_cost_matrix(align_cents(g, shift), Mc, uv_cost, cap), W)
    assert idx is not None, "a band with n_c <= W n_t is connected"
    src = g[idx]
    scale = np.float32(2.0 ** (float(shift) / 12.0))
    out = np.where(src > 0, src * scale, np.float32(0)).astype(np.float32)
    return out, idx.astype(np.int32), cost, 0


@torch.no_grad()
def contour_align_device(f0_hz, lens_c, midi, lens_t, T, band=None, shift=0.0):
    """f0_hz fp32 [B, Lc] on the device (Hz, 0 = unvoiced), lens_c [B] valid guide frames (host ints or a device tensor; None = Lc), midi int64 [B, >= T]
    on the device (the score's note per frame, 0 = rest), lens_t int32 [B] ON THE DEVICE (score frames per item: no host sync), band = half-width in
    guide frames (None or <= 0: full) -> (out [B, T] fp32, idx [B, T] int32, cost [B] int32, status [B] int32): `contour_align` of every item
    (`ss_contour_align`), frames >= lens_t[b] are out = 0, idx = -1. status 1 = not aligned (the linear fit instead): see `contour_align`.
    The direction workspace is allocated here from the library's query; sizes beyond ALIGN_MAX_T / ALIGN_MAX_LC and a workspace above
    ALIGN_MAX_WORKSPACE_BYTES are refused."""
    if not torch.is_tensor(f0_hz) or f0_hz.device.type != "cuda" or not torch.is_tensor(midi) or midi.device.type != "cuda":
        raise L.StyleSingerHipError("contour_align_device needs device tensors: there is no CPU path")
    x = f0_hz if f0_hz.dtype == torch.float32 and f0_hz.stride(1) == 1 and f0_hz.stride(0) >= f0_hz.shape[1] else f0_hz.float().contiguous()
    B, Lc = x.shape
    T = int(T)
    dev = x.device
    if T > ALIGN_MAX_T or Lc > ALIGN_MAX_LC:
        raise ValueError(f"contour_align_device: {T} score frames / {Lc} guide frames exceed the kernel's caps ({ALIGN_MAX_T} / {ALIGN_MAX_LC}); "
                         "cut the score into segments (sing_score) or use the linear fit")
    md = midi if midi.dtype == torch.int64 and midi.dim() == 2 and midi.stride(1) == 1 and midi.stride(0) >= midi.shape[1] else midi.long().contiguous()
    if md.dim() != 2 or md.shape[0] != B or md.shape[1] < T:
        raise ValueError(f"contour_align_device: midi {tuple(md.shape)} for {B} contours and {T} frames")
    lc = torch.full((B,), Lc, dtype=torch.int32) if lens_c is None else torch.as_tensor(lens_c)
    lc = lc.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    lt = lens_t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if lc.numel() != B or lt.numel() != B:
        raise ValueError(f"contour_align_device: {lc.numel()} source lengths and {lt.numel()} target lengths for {B} contours")
    band = 0 if band is None or int(band) <= 0 else int(band)
    lib = L.load()
    ws_bytes = int(lib.ss_contour_align_workspace_bytes(B, T, Lc, band))
    if ws_bytes <= 0:
        raise L.StyleSingerHipError(f"ss_contour_align_workspace_bytes refused B={B} T={T} Lc={Lc} band={band}")
    if ws_bytes > ALIGN_MAX_WORKSPACE_BYTES:
        raise ValueError(f"contour_align_device: {ws_bytes} bytes of direction workspace for B={B} T={T} Lc={Lc} band={band or 'full'} exceed "
                         f"ALIGN_MAX_WORKSPACE_BYTES = {ALIGN_MAX_WORKSPACE_BYTES}; narrow the band or split the batch")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.empty(B, T, device=dev, dtype=torch.float32)
    idx = torch.empty(B, T, device=dev, dtype=torch.int32)
    cost = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    L.ops.ss_contour_align(x, x.stride(0), Lc, lc, md, md.stride(0), lt, band, ALIGN_UV_COST, ALIGN_CAP, float(shift), out, out.stride(0), idx, cost,
                           status, T, B, ws, ws_bytes)
    return out, idx, cost, status


# ---- the score on the guide's clock (forward(pitch_timing="guide")) -------------------------------------------------------------------------------
def retime_to_guide(mel2ph, midi, idx, status_align, n_c, Lc=None):
    """The definition of the retiming (one item, integers only): the score's phones laid out on the guide's frame axis.
    mel2ph [n_t] (1-based phone per score frame), midi [n_t] (the score's note per frame, what ss_gather_expand_i64(note, mel2ph) gives), idx [n_t] and
    status_align as `contour_align` returned them for the (shifted) guide, n_c = valid guide frames, Lc >= n_c = width of the output (default n_c).
      1. score cents as contour_align: Mc[i] = 100 min(midi[i], 127) for midi[i] > 0, else ALIGN_UNVOICED;
      2. anchors a_0 = 0, every i in [1, n_t) with Mc[i] != Mc[i-1], a_m = n_t: m spans. The path is pitch-only DTW: inside a held note and between
         repeated equal notes it carries no timing, and with the tie order up, left, diagonal only the first row of a new pitch has a meaningful
         smallest j - so anchors are taken there alone and everything between them is interpolated;
      3. guide positions g_0 = 0, g_k = idx[a_k] (0 < k < m), g_m = n_c;
      4. at least one guide frame per span: h_k = g_k - k; h_k <- max(h_0 .. h_k) for k < m, the end h_m = n_c - m staying pinned (a prefix maximum
         that included it could push g_m beyond n_c when the guide crowds the last notes); then h_k <- min(h_k .. h_m); g_k = h_k + k. For n_c >= m:
         g_0 = 0, g_m = n_c, g_(k+1) - g_k >= 1 (asserted);
      5. guide frame j in span k, r = g_(k+1) - g_k, s = a_(k+1) - a_k, x = j - g_k: src[j] = a_k + ((2 x + 1) s) // (2 r) (the frame-centre rule of
         contour_fit / align_band_centres), mel2ph'[j] = mel2ph[src[j]];
      6. NOT retimed, status 1: status_align == 1, or n_c < m, or n_t == 0, or n_c == 0. Then one span [0, n_t) -> [0, n_c), the linear stretch; an
         empty item gives mel2ph' = 0, src = -1. Otherwise status 0;
      7. j >= n_c: mel2ph' = 0, src = -1.
    -> (mel2ph' int64 [Lc], src int32 [Lc], status, n_spans = m; 0 when n_t == 0)."""
    mp = np.asarray(mel2ph, dtype=np.int64)
    md = np.asarray(midi, dtype=np.int64)
    n_t, n_c = len(mp), int(n_c)
    Lc = n_c if Lc is None else int(Lc)
    assert len(md) == n_t and 0 <= n_c <= Lc
    out, src = np.zeros(Lc, dtype=np.int64), np.full(Lc, -1, dtype=np.int32)
    if n_t == 0:
        return out, src, 1, 0
    Mc = np.where(md > 0, 100 * np.minimum(md, 127), ALIGN_UNVOICED)
    a = np.concatenate([[0], 1 + np.flatnonzero(Mc[1:] != Mc[:-1]), [n_t]]).astype(np.int64)
    m = len(a) - 1
    if n_c == 0:
        return out, src, 1, m
    status = 1 if int(status_align) != 0 or n_c < m else 0
    if status:
        a, g = np.asarray([0, n_t], dtype=np.int64), np.asarray([0, n_c], dtype=np.int64)
    else:
        k = np.arange(m + 1, dtype=np.int64)
        g = np.concatenate([[0], np.asarray(idx, dtype=np.int64)[a[1:m]], [n_c]])
        h = g - k
        h[:m] = np.maximum.accumulate(h[:m])
        h = np.minimum.accumulate(h[::-1])[::-1]
        g = h + k
        assert g[0] == 0 and g[m] == n_c and (np.diff(g) >= 1).all(), "n_c >= m leaves every span a guide frame"
    j = np.arange(n_c, dtype=np.int64)
    span = np.searchsorted(g, j, side="right") - 1
    r, s, x = (g[1:] - g[:-1])[span], (a[1:] - a[:-1])[span], j - g[span]
    src[:n_c] = a[span] + ((2 * x + 1) * s) // (2 * r)
    out[:n_c] = mp[src[:n_c]]
    return out, src, status, m


@torch.no_grad()
def retime_device(mel2ph, lens_t, midi, idx, status_align, lens_c, Lc):
    """mel2ph int64 [B, >= T] and midi int64 [B, >= T] on the device, idx int32 [B, T] / status_align int32 [B] as `contour_align_device` returned them,
    lens_t int32 [B] ON THE DEVICE (score frames per item: no host sync), lens_c [B] valid guide frames (host ints or a device tensor; None = Lc),
    Lc = the guide's width -> (mel2ph' int64 [B, Lc], src int32 [B, Lc], status int32 [B], n_spans int32 [B]): `retime_to_guide` of every item
    (`ss_retime_mel2ph`). status 1 = not retimed (the linear stretch): see `retime_to_guide`. Sizes beyond ALIGN_MAX_T / ALIGN_MAX_LC are refused."""
    if not all(torch.is_tensor(t) and t.device.type == "cuda" for t in (mel2ph, midi, idx, status_align)):
        raise L.StyleSingerHipError("retime_device needs device tensors: there is no CPU path")
    B, T = idx.shape
    Lc = int(Lc)
    dev = idx.device
    if T > ALIGN_MAX_T or Lc > ALIGN_MAX_LC:
        raise ValueError(f"retime_device: {T} score frames / {Lc} guide frames exceed the kernel's caps ({ALIGN_MAX_T} / {ALIGN_MAX_LC}); "
                         "cut the score into segments (sing_score)")
    rows = lambda t: t if t.dtype == torch.int64 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.long().contiguous()
    mp, md = rows(mel2ph), rows(midi)
    for name, t in (("mel2ph", mp), ("midi", md)):
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] < T:
            raise ValueError(f"retime_device: {name} {tuple(t.shape)} for an alignment of {B} items and {T} frames")
    ix = idx.to(torch.int32).contiguous()
    sa = status_align.to(torch.int32).reshape(-1).contiguous()
    lc = torch.full((B,), Lc, dtype=torch.int32) if lens_c is None else torch.as_tensor(lens_c)
    lc = lc.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    lt = lens_t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if lc.numel() != B or lt.numel() != B or sa.numel() != B:
        raise ValueError(f"retime_device: {lc.numel()} guide lengths, {lt.numel()} score lengths and {sa.numel()} alignment states for {B} items")
    out = torch.empty(B, Lc, device=dev, dtype=torch.int64)
    src = torch.empty(B, Lc, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    n_spans = torch.empty(B, device=dev, dtype=torch.int32)
    L.ops.ss_retime_mel2ph(mp, mp.stride(0), md, md.stride(0), ix, sa, lt, lc, out, out.stride(0), src, status, n_spans, T, Lc, B)
    return out, src, status, n_spans


# ---- pitch expression controls (forward(pitch_correct=, vibrato_scale=, vibrato_add=, pitch_smooth_ms=)) ------------------------------------------
# The trend / vibrato split below is this project's own definition - a Hann moving average over the sung neighbourhood of a frame - not any tool's.
EDIT_K0 = float(1200.0 * np.log2(440.0))   # cents of A4 on the 1200 log2(Hz) axis: passed to the kernel, not restated there
EDIT_TILE, EDIT_MAX_W = L.PITCH_EDIT_TILE, L.PITCH_EDIT_MAX_W   # frames per workgroup / the widest half-window the kernel's LDS halo holds


def edit_weights(W):
    """w_k = 0.5 (1 + cos(pi k / (W + 1))), k = -W .. W, float64 [2 W + 1]: a Hann window without its zero end points."""
    k = np.arange(-int(W), int(W) + 1, dtype=np.float64)
    return 0.5 * (1.0 + np.cos(np.pi * k / (int(W) + 1)))


def _runs_of(key):
    """(lo, hi) int64 [n]: bounds [lo, hi) of the maximal run of equal `key` around every frame."""
    n = len(key)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    return np.repeat(starts, ends - starts), np.repeat(ends, ends - starts)


def held_runs(midi):
    """run_lo / run_hi int32 [n] (= a, e of the held run [a, e): a maximal run of sung frames with equal min(midi, 127)); -1 on unsung frames."""
    m = np.asarray(midi, dtype=np.int64)
    key = np.where(m > 0, np.minimum(m, 127), 0)
    lo, hi = _runs_of(key)
    return np.where(key > 0, lo, -1).astype(np.int32), np.where(key > 0, hi, -1).astype(np.int32)


def pitch_edit_parts(f, midi, W, alpha=0.0, kappa=1.0, vibrato=None, fps=None, descending=False, cents=None):
    """Every intermediate of `pitch_edit` (one item, float64 [n] each): x, c, m, nbar, s, xe (= x'), the bool mask `sung`, run_lo / run_hi.
    descending=True adds the window sums in descending k instead (tests: how much the order of the sums can move a result); cents = x given
    directly in float64 instead of 1200 f (the window's response to a pure tone, free of the input's fp32 grid; `pitch_edit` never passes it)."""
    f = np.asarray(f, dtype=np.float32)
    md = np.asarray(midi, dtype=np.int64)
    n, W = len(f), int(W)
    if len(md) != n or W < 1:
        raise ValueError(f"pitch_edit: {n} frames, {len(md)} notes, W={W}")
    if not 0.0 <= float(alpha) <= 1.0 or not float(kappa) >= 0.0:
        raise ValueError(f"pitch_edit: alpha={alpha} outside [0, 1] or kappa={kappa} < 0")
    alpha, kappa = np.float64(alpha), np.float64(kappa)
    key = np.where(md > 0, np.minimum(md, 127), 0)
    sung = key > 0
    t = np.arange(n, dtype=np.int64)
    reg_lo, reg_hi = _runs_of(sung)
    run_lo, run_hi = held_runs(md)
    x = np.where(sung, 1200.0 * f.astype(np.float64) if cents is None else np.asarray(cents, dtype=np.float64), 0.0)
    c = EDIT_K0 + 100.0 * (key - 69).astype(np.float64)
    left, right = np.minimum(W, t - reg_lo), np.minimum(W, reg_hi - 1 - t)   # how far the window reaches inside the region
    w = edit_weights(W)
    xp, cp = np.pad(x, W), np.pad(c, W)
    sx, sc, sw = np.zeros(n), np.zeros(n), np.zeros(n)
    for k in (range(W, -W - 1, -1) if descending else range(-W, W + 1)):
        on = sung & (k >= -left) & (k <= right)
        wk = w[k + W]
        sx = np.where(on, sx + wk * xp[W + k:W + k + n], sx)
        sc = np.where(on, sc + wk * cp[W + k:W + k + n], sc)
        sw = np.where(on, sw + wk, sw)
    den = np.where(sung, sw, 1.0)
    m, nbar = sx / den, sc / den
    s = np.zeros(n)
    if vibrato is not None and float(vibrato[1]) > 0:
        rate_hz, depth, delay, fade = float(vibrato[0]), np.float64(vibrato[1]), int(vibrato[2]), int(vibrato[3])
        if fps is None or delay < 0 or fade < 1:
            raise ValueError(f"pitch_edit: vibrato = (rate_hz, depth_cents, delay_frames >= 0, fade_frames >= 1) and fps (got {vibrato}, fps={fps})")
        omega = vibrato_omega(rate_hz, fps)
        a, e = run_lo.astype(np.int64), run_hi.astype(np.int64)
        o = a + delay
        on = sung & (e - a >= delay + 2 * fade) & (t >= o)
        up = np.minimum(1.0, (t - o + 1).astype(np.float64) / np.float64(fade))
        down = np.minimum(1.0, (e - t).astype(np.float64) / np.float64(fade))
        s = np.where(on, depth * up * down * np.sin((t - o).astype(np.float64) * omega), 0.0)
    xe = ((m + alpha * (nbar - m)) + kappa * (x - m)) + s
    return dict(x=x, c=c, m=m, nbar=nbar, s=s, xe=xe, sung=sung, run_lo=run_lo, run_hi=run_hi)


def vibrato_omega(rate_hz, fps):
    """Radians per frame of the synthetic vibrato, float64: what the host passes to the kernel."""
    return float(2.0 * np.pi * float(rate_hz) / float(fps))


def pitch_edit(f, midi, W, alpha=0.0, kappa=1.0, vibrato=None, u=None, fps=None):
    """The definition of the pitch edit (one item, float64): f fp32 [n] = log2 Hz (pitch_pred[..., 0]: continuous through unvoiced frames), midi int64
    [n] = the score's note per frame (0 = rest), W >= 1 the half-width of the trend window in frames, alpha in [0, 1] the correction, kappa >= 0 the
    vibrato scale, vibrato = None | (rate_hz, depth_cents, delay_frames, fade_frames >= 1) with fps = frames per second, u [n] (> 0 = unvoiced; None:
    all voiced) for the statistics only.
      * a frame is SUNG when midi[t] > 0, and VOICED when additionally not u[t] > 0; a REGION is a maximal run of sung frames, a HELD RUN [a, e) a
        maximal run of sung frames with equal min(midi, 127);
      * cents x[t] = 1200 float64(f[t]); note cents c[t] = EDIT_K0 + 100 (min(midi[t], 127) - 69);
      * weights w_k = 0.5 (1 + cos(pi k / (W + 1))), k = -W .. W (`edit_weights`); window K(t) = {k : |k| <= W and t + k in the region of t}: cut at
        rests and item ends, renormalised by the weights present;
      * trend m[t] = sum_K w_k x[t + k] / sum_K w_k, target nbar[t] the same average of c (it glides over the window instead of stepping at note
        changes); all sums in ascending k;
      * synthetic vibrato: on a held run with e - a >= delay + 2 fade, o = a + delay, for t >= o:
        s[t] = depth min(1, (t - o + 1) / fade) min(1, (e - t) / fade) sin((t - o) omega), omega = 2 pi rate_hz / fps; elsewhere s = 0;
      * x'[t] = m + alpha (nbar - m) + kappa (x - m) + s; f'[t] = fl32(x'[t] / 1200) on sung frames, f'[t] = f[t] bit for bit elsewhere. With
        alpha = 0, kappa = 1 and no vibrato f' = f bit for bit: m + (x - m) is within 2^-52 relative of the fp32 value it came from;
      * stats float64 [6] over the voiced sung frames: their count; rms of x - m (vibrato depth, cents); mean of m - nbar (sharp / flat); mean of
        |m - nbar|; max |x' - x| over ALL sung frames; count of voiced sung frames with s != 0.
    -> (f' fp32 [n], stats float64 [6], run_lo int32 [n], run_hi int32 [n]) (the held-run bounds, -1 on unsung frames)."""
    f = np.asarray(f, dtype=np.float32)
    p = pitch_edit_parts(f, midi, W, alpha, kappa, vibrato, fps)
    sung = p["sung"]
    out = f.copy()
    out[sung] = (p["xe"][sung] / 1200.0).astype(np.float32)
    voiced = sung if u is None else sung & ~(np.asarray(u) > 0)
    cnt = int(voiced.sum())
    d, q = (p["x"] - p["m"])[voiced], (p["m"] - p["nbar"])[voiced]
    stats = np.array([cnt, np.sqrt(np.sum(d * d) / cnt) if cnt else 0.0, np.sum(q) / cnt if cnt else 0.0, np.sum(np.abs(q)) / cnt if cnt else 0.0,
                      np.max(np.abs(p["xe"] - p["x"])[sung], initial=0.0), int((p["s"][voiced] != 0).sum())], dtype=np.float64)
    return out, stats, p["run_lo"], p["run_hi"]


_edit_tables = {}


def _edit_weights_device(W, dev):
    key = (int(W), str(dev))
    if key not in _edit_tables:
        _edit_tables[key] = torch.from_numpy(edit_weights(W)).to(dev)
    return _edit_tables[key]


@torch.no_grad()
def pitch_edit_device(f, u, midi, lens, W, alpha, kappa, vibrato=None, fps=None):
    """f fp32 [B, T] (log2 Hz), u fp32 [B, T] (> 0 = unvoiced), midi int64 [B, >= T] (the score's note per frame), lens int32 [B] ON THE DEVICE (None
    = T): `pitch_edit` of every item (`ss_pitch_edit_runs` + `ss_pitch_edit`). vibrato = None | (rate_hz, depth_cents, delay_frames, fade_frames)
    with fps. -> (f' fp32 [B, T], stats float64 [B, 6], run_lo int32 [B, T], run_hi int32 [B, T]). Rows may be strided (f and u with the same
    row stride; f' then has it too). No host sync; the weight table of a W is uploaded once per device. A NEUTRAL edit (alpha = 0, kappa = 1, no
    vibrato or depth 0) launches and allocates nothing: (f, None, None, None). ValueError on bad arguments, before anything is launched."""
    if not all(torch.is_tensor(t) and t.device.type == "cuda" for t in (f, u, midi)):
        raise L.StyleSingerHipError("pitch_edit_device needs device tensors: there is no CPU path")
    W, alpha, kappa = int(W), float(alpha), float(kappa)
    if f.dim() != 2 or tuple(u.shape) != tuple(f.shape):
        raise ValueError(f"pitch_edit_device: f {tuple(f.shape)} and u {tuple(u.shape)}: expected [B, T] twice")
    B, T = f.shape
    if midi.dim() != 2 or midi.shape[0] != B or midi.shape[1] < T:
        raise ValueError(f"pitch_edit_device: midi {tuple(midi.shape)} for {B} items and {T} frames")
    if not 1 <= W <= EDIT_MAX_W:
        raise ValueError(f"pitch_edit_device: W={W} outside [1, {EDIT_MAX_W}] (refused, never truncated)")
    if not 0.0 <= alpha <= 1.0 or not (kappa >= 0.0 and np.isfinite(kappa)):
        raise ValueError(f"pitch_edit_device: alpha={alpha} outside [0, 1] or kappa={kappa} < 0")
    depth, omega, delay, fade = 0.0, 0.0, 0, 1
    if vibrato is not None:
        rate, depth, delay, fade = float(vibrato[0]), float(vibrato[1]), int(vibrato[2]), int(vibrato[3])
        if fps is None or not rate > 0 or not 0.0 <= depth <= 1200.0 or delay < 0 or fade < 1:
            raise ValueError(f"pitch_edit_device: vibrato = (rate_hz > 0, depth_cents in [0, 1200], delay_frames >= 0, fade_frames >= 1) and fps "
                             f"(got {vibrato}, fps={fps})")
        omega = vibrato_omega(rate, fps)
    if lens is not None and (not torch.is_tensor(lens) or lens.numel() != B):
        raise ValueError(f"pitch_edit_device: lens must be a device tensor of {B} lengths")
    if alpha == 0.0 and kappa == 1.0 and depth == 0.0:
        return f, None, None, None
    dev = f.device
    rows = lambda t, dt: t.dtype == dt and t.stride(1) == 1 and t.stride(0) >= t.shape[1]
    if not (rows(f, torch.float32) and rows(u, torch.float32) and f.stride(0) == u.stride(0)):
        f, u = f.float().contiguous(), u.float().contiguous()
    md = midi if rows(midi, torch.int64) else midi.long().contiguous()
    lt = None if lens is None else lens.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    ld = f.stride(0)
    out = torch.empty(B, ld, device=dev, dtype=torch.float32)[:, :T]
    run_lo = torch.empty(B, T, device=dev, dtype=torch.int32)
    run_hi = torch.empty(B, T, device=dev, dtype=torch.int32)
    n_tiles = (T + EDIT_TILE - 1) // EDIT_TILE
    partial = torch.empty(B, n_tiles, 6, device=dev, dtype=torch.float64)
    stats = torch.empty(B, 6, device=dev, dtype=torch.float64)
    L.ops.ss_pitch_edit_runs(md, md.stride(0), lt, run_lo, run_hi, T, B)
    L.ops.ss_pitch_edit(f, ld, md, md.stride(0), u, lt, run_lo, run_hi, _edit_weights_device(W, dev), W, EDIT_K0, alpha, kappa, depth, omega, delay, fade,
                        out, partial, stats, T, B)
    return out, stats, run_lo, run_hi
