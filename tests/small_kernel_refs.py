"""Plain float64 statements of the small encoder-side and producer ops, written from each op's definition
(include/stylesinger_hip.h and the reference lines it cites), for tests/test_gpu_small_kernels.py.

numpy only: no GPU, no HIP library. tests/test_small_kernel_refs_cpu.py checks these statements themselves against torch /
numpy / the oracle, so that a wrong reference cannot pass a wrong kernel. The two input generators at the end are shared by the
CPU test (which asserts their conditions in float64) and the GPU test (which feeds them to the kernels).
"""
import numpy as np

F64 = np.float64


# ------------------------------------------------------------------------------------------------
# attention / layernorm / LSTM / norms
# ------------------------------------------------------------------------------------------------
def attention(q, k, v, *, H, D, scale, qlens=None, klens=None):
    """q [B,Tq,H*D], k / v [B,Tk,H*D] -> (out [B,Tq,H*D], written [B,Tq] bool). Explicit softmax over k < klen per (b, head);
    rows q >= qlen are 'left untouched' (written = False, out 0 there); an item without keys gives zeros."""
    q, k, v = (np.asarray(a, F64) for a in (q, k, v))
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    out = np.zeros((B, Tq, H * D), F64)
    written = np.zeros((B, Tq), bool)
    for b in range(B):
        m = Tq if qlens is None else min(int(qlens[b]), Tq)
        n = Tk if klens is None else min(int(klens[b]), Tk)
        written[b, :m] = True
        if n == 0:
            continue
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            s = (q[b, :m, c] @ k[b, :n, c].T) * scale
            p = np.exp(s - s.max(-1, keepdims=True))
            out[b, :m, c] = (p / p.sum(-1, keepdims=True)) @ v[b, :n, c]
    return out, written


def layernorm(x, gamma, beta, eps=1e-5, lens=None, mask_rows=False):
    """x [B,T,C]: (x - mean) / sqrt(var + eps) * gamma + beta with the biased variance; rows t >= lens[b] are 0 when mask_rows and lens are given."""
    x = np.asarray(x, F64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps) * np.asarray(gamma, F64) + np.asarray(beta, F64)
    if mask_rows and lens is not None:
        y = y * (np.arange(x.shape[1])[None, :] < np.asarray(lens)[:, None])[..., None]
    return y


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_layer(xproj, w_hh):
    """One LSTM layer from zero state. xproj [P,n,4H] = x_t W_ih^T + b_ih + b_hh in torch's row order (gate-major: i, f, g, o blocks of H),
    w_hh [4H,H]. -> h_seq [P,n,H]."""
    xproj, w_hh = np.asarray(xproj, F64), np.asarray(w_hh, F64)
    P, n, H4 = xproj.shape
    H = H4 // 4
    h = np.zeros((P, H), F64)
    c = np.zeros((P, H), F64)
    out = np.zeros((P, n, H), F64)
    for t in range(n):
        a = xproj[:, t] + h @ w_hh.T
        i, f, g, o = _sigmoid(a[:, :H]), _sigmoid(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        out[:, t] = h
    return out


def interleave_gates(xproj):
    """[P,n,4H] gate-major -> [P,n,H,4]: the (i, f, g, o)-per-hidden-unit order ss_lstm_layer reads (pure re-indexing)."""
    P, n, H4 = xproj.shape
    return np.ascontiguousarray(xproj.reshape(P, n, 4, H4 // 4).transpose(0, 1, 3, 2))


def mean_l2norm(x):
    m = np.asarray(x, F64).mean(0)
    return m / np.sqrt((m * m).sum())


def l2norm_rows(x):
    x = np.asarray(x, F64)
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


# ------------------------------------------------------------------------------------------------
# positions / length regulator / gathers / lookups
# ------------------------------------------------------------------------------------------------
def make_positions(nz):
    nz = np.asarray(nz).astype(np.int64)
    return np.cumsum(nz, axis=1) * nz


def round_half_even(x):
    return np.rint(np.asarray(x, F64))


def length_regulate(logdur, tokens, Tmax):
    """-> (dur [B,Tp] int64, mel2ph [B,Tmax] int64 or None when Tmax == 0, lens [B] int64)."""
    logdur, tokens = np.asarray(logdur, F64), np.asarray(tokens)
    dur = np.maximum(round_half_even(np.exp(logdur) - 1.0), 0.0).astype(np.int64)
    dur[tokens == 0] = 0
    tot = dur.sum(1)
    if Tmax == 0:
        return dur, None, tot
    B, Tp = dur.shape
    mel2ph = np.zeros((B, Tmax), np.int64)
    for b in range(B):
        frames = np.repeat(np.arange(1, Tp + 1), dur[b])[:Tmax]
        mel2ph[b, :len(frames)] = frames
    return dur, mel2ph, np.minimum(tot, Tmax)


def gather_expand(src, mel2ph):
    """src [B,Tsrc(,C)], mel2ph [B,T]: out[b,t] = src[b, m-1] where 0 < m <= Tsrc, else 0."""
    src, mel2ph = np.asarray(src), np.asarray(mel2ph)
    B, Tsrc = src.shape[:2]
    ok = (mel2ph > 0) & (mel2ph <= Tsrc)
    idx = np.where(ok, mel2ph - 1, 0)
    out = src[np.arange(B)[:, None], idx]
    out[~ok] = 0
    return out


def embedding(idx, table, scale, prev=None):
    """scale * table[clip(idx, 0, n-1)] (+ prev), float64."""
    table = np.asarray(table, F64)
    out = F64(scale) * table[np.clip(np.asarray(idx), 0, table.shape[0] - 1)]
    return out if prev is None else out + np.asarray(prev, F64)


def table_add(pos, table, alpha, prev=None):
    """alpha * table[min(pos, rows-1)] (+ prev), float64."""
    table = np.asarray(table, F64)
    out = F64(alpha) * table[np.minimum(np.asarray(pos), table.shape[0] - 1)]
    return out if prev is None else out + np.asarray(prev, F64)


def add_bcast_mask(x, v1=None, y1=None, v2=None, y2=None, lens=None, dtype=F64):
    """((((x + v1[b]) + y1) + v2[b]) + y2) * (t < lens[b]) in `dtype`, every step rounded to it (float32 = the documented fp32 sum)."""
    out = np.asarray(x, dtype).copy()
    if v1 is not None:
        out = out + np.asarray(v1, dtype)[:, None, :]
    if y1 is not None:
        out = out + np.asarray(y1, dtype)
    if v2 is not None:
        out = out + np.asarray(v2, dtype)[:, None, :]
    if y2 is not None:
        out = out + np.asarray(y2, dtype)
    if lens is not None:
        out[np.arange(out.shape[1])[None, :] >= np.asarray(lens)[:, None]] = 0
    return out


def note_dur_add(prev, dur, w, b):
    return np.asarray(prev, F64) + np.asarray(dur, F64)[:, None] * np.asarray(w, F64)[None, :] + np.asarray(b, F64)[None, :]


def add_rowscalar(x, s, lens=None):
    x, s = np.asarray(x, F64), np.asarray(s, F64)
    keep = np.ones(x.shape[:2], bool) if lens is None else np.arange(x.shape[1])[None, :] < np.asarray(lens)[:, None]
    return x + s[..., None] * keep[..., None]


def mask_rows_by_ref(x, ref_col):
    out = np.array(x, copy=True)
    out[np.asarray(ref_col) == 0] = 0
    return out


def count_positive(x):
    return (np.asarray(x) > 0).sum(1)


def ref_lens(ref_mels):
    """1 + last t with ref_mels[b,t,0] != 0, 0 when there is none."""
    nz = np.asarray(ref_mels)[:, :, 0] != 0
    T = nz.shape[1]
    return np.where(nz.any(1), T - np.argmax(nz[:, ::-1], axis=1), 0)


# ------------------------------------------------------------------------------------------------
# pitch (modules/StyleSinger/stylesinger.py:255-311, utils/pitch_utils.py:14-31,65-78 of the reference)
# ------------------------------------------------------------------------------------------------
F0_MEL_MIN = 1127 * np.log(1 + 50.0 / 700)
F0_MEL_MAX = 1127 * np.log(1 + 1100.0 / 700)


def f0_bounds(midi):
    """dyn_clip bounds: minmax_norm(log2(440 * 2^((midi -+ 3 - 69) / 12))), log2 clamped at 10, result clamped to [-1, 1]."""
    midi = np.asarray(midi, F64)

    def norm(note):
        x = np.minimum(np.log2(2.0 ** ((note - 69.0) / 12.0) * 440.0), 10.0)
        return np.clip((x - 6.0) / (10.0 - 6.0) * 2.0 - 1.0, -1.0, 1.0)
    return norm(midi - 3.0), norm(midi + 3.0)


def coarse_coordinate(hz):
    """f0_to_coarse before its final (. + 0.5).long(): the bin coordinate in [1, 255]."""
    hz = np.asarray(hz, F64)
    mel = 1127 * np.log(1 + hz / 700)
    pos = mel > 0
    mel[pos] = (mel[pos] - F0_MEL_MIN) * 254 / (F0_MEL_MAX - F0_MEL_MIN) + 1
    mel[mel <= 1] = 1
    mel[mel > 255] = 255
    return mel


def f0_to_coarse(hz):
    return np.floor(coarse_coordinate(hz) + 0.5).astype(np.int64)


def pitch_post(f0_a, uv_a, f0_b, uv_b, midi, mel2ph):
    """-> (pitch_pred [n,2], f0_denorm [n], coarse [n] int64, coordinate [n]). uv forced to 1 on rests (midi == 0); both predictors
    minmax-denormed to log2 Hz and averaged as b/2 + a/2; Hz = 2^f, 0 where uv > 0 or mel2ph == 0."""
    rest = np.asarray(midi) == 0
    ua = np.where(rest, 1.0, (np.asarray(uv_a) != 0).astype(F64))
    ub = np.where(rest, 1.0, (np.asarray(uv_b) != 0).astype(F64))
    fa = (np.asarray(f0_a, F64) + 1) / 2 * (10 - 6) + 6
    fb = (np.asarray(f0_b, F64) + 1) / 2 * (10 - 6) + 6
    f = fb / 2 + fa / 2
    u = ub / 2 + ua / 2
    hz = 2.0 ** f
    hz[(u > 0) | (np.asarray(mel2ph) == 0)] = 0.0
    coord = coarse_coordinate(hz)
    return np.stack([f, u], -1), hz, np.floor(coord + 0.5).astype(np.int64), coord


def coarse_band(coord, width=1e-3):
    """True where the float64 bin coordinate is within `width` of a .5 boundary (a last-bit fp32 difference may flip the bin there)."""
    return np.abs(coord - np.floor(coord) - 0.5) < width


# ------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------
def spec_magnitude(S, nbins, sin_off, ldp, power=False):
    """S [rows,lds] = (re | im) column blocks -> [rows,ldp]: |X| (or |X|^2) in the first nbins columns, 0 in the rest."""
    S = np.asarray(S, F64)
    re, im = S[:, :nbins], S[:, sin_off:sin_off + nbins]
    p = re * re + im * im
    out = np.zeros((S.shape[0], ldp), F64)
    out[:, :nbins] = p if power else np.sqrt(p)
    return out


def reflect_pad(x, lens, Ly, pad):
    """x [B,Lx] -> [B,Ly]: numpy.pad(mode="reflect") of each item's first lens[b] samples, zeros beyond n + 2 pad (an empty item is all zeros)."""
    x = np.asarray(x)
    out = np.zeros((x.shape[0], Ly), x.dtype)
    for b in range(x.shape[0]):
        n = int(lens[b])
        if n > 0:
            out[b, :n + 2 * pad] = np.pad(x[b, :n], pad, mode="reflect")
    return out


def log10_floor(x, eps):
    return np.log10(np.maximum(np.asarray(x, F64), F64(eps)))


def normalize_volume_gain(wav, lens, target_dbfs):
    """normalize_volume(increase_only=True): gain[b] = 10^(change / 20), change = target - 10 log10(mean(wav[b,:lens[b]]^2)), when change >= 0; else 1.
    An empty or silent item keeps gain 1."""
    wav = np.asarray(wav, F64)
    gain = np.ones(wav.shape[0], F64)
    for b in range(wav.shape[0]):
        n = int(np.clip(lens[b], 0, wav.shape[1]))
        ms = (wav[b, :n] ** 2).mean() if n > 0 else 0.0
        if ms > 0:
            change = target_dbfs - 10 * np.log10(ms)
            if change >= 0:
                gain[b] = 10 ** (change / 20)
    return gain


def round_f16_rows(x, n_in, n_out, ldy):
    """x [B,Lx] fp32 -> [B,ldy] fp32: the fp16 round trip of the first min(n_out, n_in, Lx) samples, 0 in the other columns."""
    x = np.asarray(x, np.float32)
    out = np.zeros((x.shape[0], ldy), np.float32)
    for b in range(x.shape[0]):
        n = min(int(n_out[b]), x.shape[1] if n_in is None else int(n_in[b]), x.shape[1], ldy)
        with np.errstate(over="ignore"):
            out[b, :n] = x[b, :n].astype(np.float16).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------
# shared inputs with conditions the CPU test asserts
# ------------------------------------------------------------------------------------------------
PITCH_POST_SEED = 20
PITCH_POST_N = 1000
LR_TPS = (1, 64, 70, 150)
LR_B = 3


def pitch_post_inputs(n=PITCH_POST_N, seed=PITCH_POST_SEED):
    """f0 of both predictors spanning [-1.2, 1.2], every (uv_a, uv_b) combination, rests and mel2ph == 0 frames; the first eight frames are voiced
    non-rest frames whose two predictors agree at the ends of the range, so that both f0_to_coarse clamps (1 and 255) are hit well inside."""
    g = np.random.default_rng(seed)
    f0_a = g.uniform(-1.2, 1.2, n).astype(np.float32)
    f0_b = g.uniform(-1.2, 1.2, n).astype(np.float32)
    uv_a = (g.random(n) < 0.3).astype(np.int32)
    uv_b = (g.random(n) < 0.3).astype(np.int32)
    midi = np.where(g.random(n) < 0.15, 0, g.integers(40, 90, n)).astype(np.int64)
    mel2ph = np.where(g.random(n) < 0.1, 0, g.integers(1, 60, n)).astype(np.int64)
    f0_a[:4], f0_b[:4] = -1.2, -1.15
    f0_a[4:8], f0_b[4:8] = 1.2, 1.15
    uv_a[:8], uv_b[:8], midi[:8], mel2ph[:8] = 0, 0, 60, 1
    for j, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):   # each uv combination on a non-rest, non-pad frame
        uv_a[8 + j], uv_b[8 + j], midi[8 + j], mel2ph[8 + j] = a, b, 62, 3
    midi[12], mel2ph[12], uv_a[12], uv_b[12] = 0, 5, 0, 0            # a rest with both predictors voiced
    midi[13], mel2ph[13], uv_a[13], uv_b[13] = 64, 0, 0, 0           # a padding frame with both predictors voiced
    return f0_a, uv_a, f0_b, uv_b, midi, mel2ph


def length_regulator_inputs(Tp, B=LR_B, seed=7):
    """-> (logdur [B,Tp] fp32, tokens [B,Tp] int64, target [B,Tp] float64 = d + delta). logdur = log(1 + d + delta) with integer d in [0, 12] and
    |delta| <= 0.25, so exp(logdur) - 1 stays >= 0.25 away from every rounding tie. Item 0 also carries a negative log-duration and an exact 0,
    pad tokens in the middle; item 1 ends in pad tokens; the last item is all pad."""
    g = np.random.default_rng(seed + Tp)
    d = g.integers(0, 13, (B, Tp)).astype(F64)
    target = d + g.uniform(-0.25, 0.25, (B, Tp))
    tokens = g.integers(1, 60, (B, Tp)).astype(np.int64)
    if Tp >= 8:
        target[0, 1] = np.exp(-1.5) - 1.0     # negative log-duration: exp(x) - 1 < 0 -> 0 frames
        target[0, 2] = 0.0                    # logdur == 0 exactly
        tokens[0, 4:6] = 0                    # pads in the middle (their durations must not count)
        target[0, 4] = 5.1
        tokens[1, Tp - Tp // 4:] = 0          # pads at the end
    tokens[B - 1] = 0                         # an all-pad item
    logdur = np.log(1.0 + target).astype(np.float32)
    return logdur, tokens, target


def tie_margin(logdur):
    """distance of exp(logdur) - 1 (float64 of the fp32 input) from the nearest rounding tie k + 0.5, k >= 0. Ties below zero do not count: both
    sides of them are clamped to 0 frames."""
    v = np.exp(np.asarray(logdur, F64)) - 1.0
    m = np.abs(v - np.floor(v) - 0.5)
    return np.where(v < 0, 0.5 - v, m)
