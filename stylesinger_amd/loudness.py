"""ITU-R BS.1770 integrated loudness and loudness normalisation on the GPU: with hparams['loud_norm'] the reference normalises the reference
audio in `librosa_wav2spec` (utils/audios/__init__.py:56-61):
    meter = pyln.Meter(sr); loudness = meter.integrated_loudness(wav); wav = pyln.normalize.loudness(wav, loudness, -22.0)
    if np.abs(wav).max() > 1: wav = wav / np.abs(wav).max()
pyloudnorm (0.1.0) is an UN-VENDORED dependency of the reference, so this file restates the published algorithm - parity with pyloudnorm is
UNPINNED: there is no golden of the real package to check against, and the filter design below was written from memory of the package's
(RBJ-style biquads from G, Q, fc), not read from it. It is this module's definition, not a quote. What IS pinned: this module against an
independent restatement (tests/loudness_ref.py: scipy's lfilter per stage, literal loops), the 48 kHz coefficients against the tables of
BS.1770-4, a 997 Hz full-scale sine against -3.01 LKFS within the 0.1 LU compliance tolerance, and the kernel against the restatement within
half an fp32 ulp of the gain.

Definition (float64 on the host):
  filter   two biquads in cascade, each normalised by its a0. With w0 = 2 pi fc / rate, alpha = sin w0 / (2 Q), c = cos w0:
             high shelf, G = 4 dB, Q = 1 / sqrt 2, fc = 1500 Hz, A = 10^(G / 40), s = 2 sqrt(A) alpha:
               b = A [(A+1) + (A-1) c + s], -2 A [(A-1) + (A+1) c], A [(A+1) + (A-1) c - s]
               a =    (A+1) - (A-1) c + s,     2 [(A-1) - (A+1) c],    (A+1) - (A-1) c - s
             high pass, Q = 0.5, fc = 38 Hz:   b = (1+c) / 2, -(1+c), (1+c) / 2     a = 1 + alpha, -2 c, 1 - alpha
           At 48 kHz the shelf is within 1.1e-4 of BS.1770-4 Table 1 and the high pass' a within 2.9e-5 of Table 2; its b is
           0.99504 (1, -2, 1), not (1, -2, 1): a full-scale 997 Hz sine reads -3.0517 LKFS, not -3.01.
  blocks   mono, channel gain 1, T_g = 0.4 s, step = 0.25: nb = int(np.round((n / rate - T_g) / (T_g step)) + 1); block j covers
           [int(T_g (j step) rate), int(T_g (j step + 1) rate)) - exactly these float64 expressions. The last block may reach past n (n = 0.46
           rate): its slice is truncated, the divisor stays T_g rate: z_j = sum y^2 / (T_g rate).
  gating   l_j = -0.691 + 10 log10 z_j; J1 = {l_j >= -70}; Gamma_r = -0.691 + 10 log10(mean z over J1) - 10; J2 = {l_j > Gamma_r and l_j > -70};
           L = -0.691 + 10 log10(mean z over J2).
  gain     numpy 1.21 semantics (the version the reference pins: a float32 array times a float64 scalar stays float32):
           g32 = fl32(10^((target - L) / 20)); y = fl32(g32 x); P = fl32(g32 max|x|) = max|y| (rounding is monotone); P > 1: y = y / P (fp32).
  where the package raises or produces NaN: an item shorter than T_g rate samples is a ValueError (as pyloudnorm raises), or with
           short="skip" gain 1 and L = NaN; an item whose J1 or J2 is empty (digital silence) has L = -inf and gain 1 (the reference would
           produce a NaN mel for it).
The host statement runs the cascade as the same chunked scan the kernel runs (every chunk from zero state, carries through A^C, the
homogeneous response added from a tabulated basis), vectorised over the chunks; `ss_loudness_measure` / `ss_loudness_apply`
(csrc/loudness.hip) are the device form."""
import functools
import math

import numpy as np
import torch

from . import lib as L
from .resample import _cached

T_G = 0.4
STEP = 0.25
DEFAULT_TARGET = -22.0
DEFAULT_CHUNK = 256   # device scan: 256 chunks of 256 samples per workgroup; the carry scan then walks n / 16384 groups per item
_HOST_CHUNK = 1024


def resolve_loudness(hparams, loudness=None):
    """The opt-in: -> True when the reference audio is to be loudness-normalised. hparams['loud_norm'] alone stays refused (parity with
    pyloudnorm is unpinned: never a silent default); `loudness="bs1770"` accepts it. No device is touched."""
    if loudness not in (None, "bs1770"):
        raise ValueError(f"loudness={loudness!r}: expected None or 'bs1770'")
    want = bool(hparams and hparams.get("loud_norm"))
    if want and loudness is None:
        # process_audio passes loud_norm to librosa_wav2spec (inference/StyleSinger.py:85; utils/audios/__init__.py:55-59: pyloudnorm, un-vendored)
        raise NotImplementedError("hparams['loud_norm'] is set: the reference normalises the reference audio with pyloudnorm, which is un-vendored. "
                                  "Pass loudness=\"bs1770\" to StyleSingerInfer to use this project's BS.1770 meter (stylesinger_amd/loudness.py; "
                                  "parity with pyloudnorm is unpinned); refusing rather than computing a different mel silently")
    return want


@functools.lru_cache(maxsize=None)
def k_weighting(rate):
    """-> ((b, a) of the high shelf, (b, a) of the high pass): float64 arrays of 3, each stage normalised by its a0 (a[0] = 1)."""
    rate = float(rate)
    if not rate > 0:
        raise ValueError(f"k_weighting: the sample rate must be positive (got {rate})")

    def norm(b, a):
        b, a = np.asarray(b, dtype=np.float64) / a[0], np.asarray(a, dtype=np.float64) / a[0]
        b.setflags(write=False)
        a.setflags(write=False)
        return b, a
    w0 = 2.0 * np.pi * 1500.0 / rate
    A = 10.0 ** (4.0 / 40.0)
    alpha, c = np.sin(w0) / (2.0 * (1.0 / np.sqrt(2.0))), np.cos(w0)
    s = 2.0 * np.sqrt(A) * alpha
    shelf = norm([A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)],
                 [(A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s])
    w0 = 2.0 * np.pi * 38.0 / rate
    alpha, c = np.sin(w0) / (2.0 * 0.5), np.cos(w0)
    hp = norm([(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + alpha, -2 * c, 1 - alpha])
    return shelf, hp


def n_blocks(n, rate):
    """Gating blocks of an item of n samples; 0 when it is shorter than one block (n < T_g rate)."""
    if n < T_G * rate:
        return 0
    return int(np.round((n / rate - T_G) / (T_G * STEP)) + 1)


def block_bounds(n, rate):
    """-> int64 [nb, 2]: block j covers [lo, hi); hi of the last block may exceed n (the slice is then truncated)."""
    nb = n_blocks(n, rate)
    return np.array([[int(T_G * (j * STEP) * rate), int(T_G * (j * STEP + 1) * rate)] for j in range(nb)], dtype=np.int64).reshape(nb, 2)


def _step(coef, x, st):
    """One sample of the cascade (both stages in the transposed direct form II) for vectors of inputs / states; st [4, ...] is updated."""
    (b, a), (g, d) = coef
    y1 = b[0] * x + st[0]
    st[0] = b[1] * x - a[1] * y1 + st[1]
    st[1] = b[2] * x - a[2] * y1
    y = g[0] * y1 + st[2]
    st[2] = g[1] * y1 - d[1] * y + st[3]
    st[3] = g[2] * y1 - d[2] * y
    return y


@functools.lru_cache(maxsize=32)
def _basis(rate, C):
    """(H [C, 4]: the output at step j of a chunk started from each unit state with zero input; M [4, 4] = A^C: its state after C steps)"""
    coef = k_weighting(rate)
    st = np.eye(4)          # st[:, q] = the state started from unit vector q
    H = np.empty((C, 4))
    zero = np.zeros(4)
    for j in range(C):
        H[j] = _step(coef, zero, st)
    M = st.copy()
    H.setflags(write=False)
    M.setflags(write=False)
    return H, M


def k_filter_f64(x, rate, chunk=_HOST_CHUNK):
    """K-weighted signal, float64: the cascade over x from zero state, as a chunked scan vectorised over the chunks."""
    x = np.asarray(x, dtype=np.float64)
    n, C = len(x), int(chunk)
    nch = max(1, -(-n // C))
    X = np.zeros(nch * C)
    X[:n] = x
    X = X.reshape(nch, C)
    coef = k_weighting(rate)
    st = np.zeros((4, nch))
    Y = np.empty((nch, C))
    for j in range(C):
        Y[:, j] = _step(coef, X[:, j], st)
    H, M = _basis(rate, C)
    S = np.zeros((nch, 4))
    for c in range(nch - 1):
        S[c + 1] = M @ S[c] + st[:, c]
    Y += S @ H.T
    return Y.reshape(-1)[:n]


def loudness_details_f64(x, rate):
    """The host definition with its intermediate results: dict(L, z [nb], l [nb], J1, J2 (index arrays), bounds [nb, 2])."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n < T_G * rate:
        raise ValueError(f"integrated loudness: the item has {n} samples, fewer than one {T_G} s block at {rate} Hz")
    y2 = k_filter_f64(x, rate) ** 2
    bounds = block_bounds(n, rate)
    z = np.array([y2[lo:hi].sum() for lo, hi in bounds]) / (T_G * rate)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        J1 = np.nonzero(l >= -70.0)[0]
        Lout, J2 = -np.inf, np.zeros(0, dtype=np.int64)
        if len(J1):
            rel = -0.691 + 10.0 * np.log10(z[J1].mean()) - 10.0
            J2 = np.nonzero((l > rel) & (l > -70.0))[0]
            if len(J2):
                Lout = float(-0.691 + 10.0 * np.log10(z[J2].mean()))
    return dict(L=Lout, z=z, l=l, J1=J1, J2=J2, bounds=bounds)


def integrated_loudness_f64(x, rate):
    """BS.1770 integrated loudness of a mono signal in LUFS (float64 host definition); -inf for digital silence; ValueError when the item is
    shorter than one block."""
    return loudness_details_f64(x, rate)["L"]


def gain_f32(L_, target=DEFAULT_TARGET):
    """g32 = fl32(10^((target - L) / 20)); 1 where L is not finite."""
    return np.float32(10.0 ** ((target - L_) / 20.0)) if np.isfinite(L_) else np.float32(1.0)


def normalize_f32(x, rate, target=DEFAULT_TARGET):
    """Host statement of the normalisation for one float32 item -> (y float32, L, g32)."""
    x = np.asarray(x, dtype=np.float32)
    L_ = integrated_loudness_f64(x, rate)
    g = gain_f32(L_, target)
    y = (g * x).astype(np.float32)
    P = np.float32(g * np.abs(x).max()) if len(x) else np.float32(0)
    if P > 1:
        y = (y / P).astype(np.float32)
    return y, L_, g


# ---- device ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def device_table(rate, C):
    """The float64 table `ss_loudness_measure` reads (include/stylesinger_hip.h): coefficients, T_g rate, A^(C 2^i) for i = 0 .. 5."""
    (b, a), (g, d) = k_weighting(rate)
    _, M = _basis(rate, C)
    tab = np.zeros(12 + 6 * 16)
    tab[0:5] = [b[0], b[1], b[2], a[1], a[2]]
    tab[5:10] = [g[0], g[1], g[2], d[1], d[2]]
    tab[10] = T_G * rate
    P = np.array(M)
    for i in range(6):
        tab[12 + 16 * i:28 + 16 * i] = P.reshape(-1)
        P = P @ P
    tab.setflags(write=False)
    return tab


def segment_edges(n, rate):
    """The n_blocks + 4 ascending sample indices that cut an item into gating segments: block j = [edges[j], edges[j + 4]) (the blocks overlap
    by 75 %, so hi of block j IS lo of block j + 4), the last edge cut to n."""
    bounds = block_bounds(n, rate)
    nb = len(bounds)
    if nb == 0:
        return []
    edges = [int(T_G * (k * STEP) * rate) for k in range(nb + 4)]
    if any(edges[j] != lo or edges[j + 4] != hi for j, (lo, hi) in enumerate(bounds)):
        raise AssertionError("loudness: the gating blocks are not four whole segments each")   # (j step + 1 == (j + 4) step exactly in float64)
    edges[-1] = min(edges[-1], int(n))
    return edges


def _meta(lens, rate, C, short):
    nbs, rows = [], []
    for n in lens:
        e = segment_edges(n, rate)
        if not e and short != "skip":
            raise ValueError(f"loudness: an item has {n} samples, fewer than one {T_G} s block at {rate} Hz (short='skip' leaves such an item untouched)")
        if e and (min(np.diff(e[:-1])) < C or e[-1] <= e[-2]):
            raise ValueError(f"loudness: chunk={C} exceeds the {min(np.diff(e[:-1]))} samples between two block starts at {rate} Hz")
        nbs.append(max(0, len(e) - 4))
        rows.append(e)
    lde = max(nbs) + 4 + 1
    tbl = np.zeros((len(lens), 2 + lde), dtype=np.int32)
    for b, (n, nb, e) in enumerate(zip(lens, nbs, rows)):
        tbl[b, 0], tbl[b, 1] = n, nb
        tbl[b, 2:2 + len(e)] = e
    return tbl, nbs, lde


def _prepare(wavs, lens, rate, chunk, short, who):
    if not torch.is_tensor(wavs) or wavs.device.type != "cuda":
        raise L.StyleSingerHipError(f"{who} needs device tensors: there is no CPU path")
    if short not in ("raise", "skip"):
        raise ValueError(f"{who}: short={short!r}: expected 'raise' or 'skip'")
    rate, C = int(rate), int(DEFAULT_CHUNK if chunk is None else chunk)
    lens = [int(v) for v in lens]
    if wavs.dim() != 2 or len(lens) != wavs.shape[0]:
        raise ValueError(f"{who}: wavs must be [B, L] with one length per row (got {tuple(wavs.shape)}, {len(lens)} lengths)")
    if C < 32 or C > 4096 or C % 32:
        raise ValueError(f"{who}: chunk={C}: expected a multiple of 32 in [32, 4096]")
    x = wavs if wavs.dtype == torch.float32 and wavs.stride(1) == 1 and wavs.stride(0) >= wavs.shape[1] else wavs.float().contiguous()
    B, Lx = x.shape
    if B < 1 or Lx < 1 or B > 65535 or Lx >= 2 ** 31 or min(lens) < 0 or max(lens) > Lx:
        raise ValueError(f"{who}: lengths {lens} outside the buffer of {Lx} samples, or an empty / oversized batch")
    dev = x.device
    tab = _cached(("loud_tab", rate, C, dev), lambda: torch.from_numpy(device_table(rate, C).copy()).to(dev))

    def make():
        tbl, nbs, lde = _meta(lens, rate, C, "skip")
        t = torch.from_numpy(tbl).to(dev)
        return t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2:].contiguous(), nbs, lde
    n_d, nb_d, edges_d, nbs, lde = _cached(("loud_lens", rate, C, dev, tuple(lens)), make)
    if short == "raise" and any(nb == 0 for nb in nbs):
        _meta(lens, rate, C, "raise")
    return x, lens, rate, C, tab, n_d, nb_d, edges_d, nbs, lde


def _measure(x, rate, C, target, tab, n_d, nb_d, edges_d, nbs, lde):
    B, Lx = x.shape
    dev = x.device
    lib = L.load()
    ldz = max(1, max(nbs))
    out = dict(lufs=torch.empty(B, device=dev, dtype=torch.float64), gain=torch.empty(B, device=dev, dtype=torch.float32),
               peak=torch.empty(B, device=dev, dtype=torch.float32), z=torch.empty(B, ldz, device=dev, dtype=torch.float64), n_blocks=list(nbs))
    nbytes = int(lib.ss_loudness_workspace_bytes(B, Lx, C))
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    L.ops.ss_loudness_measure(x, x.stride(0), Lx, n_d, nb_d, edges_d, lde, B, tab, C, float(target), out["lufs"], out["gain"], out["peak"], out["z"],
                              ldz, ws, nbytes)
    return out


@torch.no_grad()
def measure_batch(wavs, lens, rate, target=DEFAULT_TARGET, chunk=None, short="raise"):
    """wavs [B, L] fp32 on the device, lens host ints (samples past lens[b] are padding, whatever they hold) -> dict of device tensors:
    lufs [B] float64 (-inf: digital silence; NaN: shorter than one block with short="skip"), gain [B] fp32 = fl32(10^((target - lufs) / 20)) (1
    where lufs is not finite), peak [B] fp32 = max |x|, z [B, max blocks] float64 (the block mean squares; 0 past an item's blocks), and
    n_blocks (host ints). After one eager call per (rate, lens) no host-to-device copy is issued: graph-capturable."""
    x, lens, rate, C, tab, n_d, nb_d, edges_d, nbs, lde = _prepare(wavs, lens, rate, chunk, short, "measure_batch")
    return _measure(x, rate, C, target, tab, n_d, nb_d, edges_d, nbs, lde)


@torch.no_grad()
def normalize_batch(wavs, lens, rate, target=DEFAULT_TARGET, chunk=None, short="raise"):
    """-> (y [B, L] fp32: every item at `target` LUFS, divided by its peak where that exceeds 1, exact zeros past lens[b];
    dict(lufs=, gain=, peak=) as `measure_batch` returns them: the INPUT's loudness, the gain applied before the peak rule, the input's max |x|)."""
    x, lens, rate, C, tab, n_d, nb_d, edges_d, nbs, lde = _prepare(wavs, lens, rate, chunk, short, "normalize_batch")
    m = _measure(x, rate, C, target, tab, n_d, nb_d, edges_d, nbs, lde)
    B, Lx = x.shape
    y = torch.empty(B, Lx, device=x.device, dtype=torch.float32)
    L.ops.ss_loudness_apply(x, x.stride(0), Lx, n_d, m["gain"], m["peak"], y, Lx, Lx, B)
    return y, dict(lufs=m["lufs"], gain=m["gain"], peak=m["peak"], n_blocks=m["n_blocks"])
