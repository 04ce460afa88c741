"""float64 numpy restatement of the WPE contract: nara-wpe's stft / istft with
fading and wpe_v6 per frequency bin, written from their published definitions, plus the
degenerate-case rules the contract adds.  precision="f32" is the precision model the GPU is held
to: STFT, lambda, the filter application and the inverse STFT in float32 / complex64 (scipy.fft
keeps single precision), R, p and the solve in float64, the output cast to float32.  Test
infrastructure, not the code under test.
"""
import numpy as np
import scipy.fft
import scipy.signal

FFT, HOP, BINS, FADE = 512, 128, 257, 384


def window():
    return scipy.signal.windows.blackman(FFT, sym=False)


def synthesis_window():
    w = window()
    den = np.zeros(FFT)
    for n in range(FFT):
        den[n] = np.sum(w[n % HOP::HOP] ** 2)
    return w / den


def num_frames(n: int) -> int:
    return -(-(n + 2 * FADE - FFT) // HOP) + 1


def _real(precision):
    return np.float32 if precision == "f32" else np.float64


def stft(x, precision="f64"):
    """x [n] -> Y [T][257]."""
    rt = _real(precision)
    x = np.asarray(x, rt)
    T = num_frames(len(x))
    pad = np.zeros(HOP * (T - 1) + FFT, rt)
    pad[FADE:FADE + len(x)] = x
    idx = HOP * np.arange(T)[:, None] + np.arange(FFT)[None, :]
    frames = pad[idx] * window().astype(rt)
    return scipy.fft.rfft(frames, axis=1)


def istft(X, n: int, precision="f64"):
    """X [T][257] -> [n]: irfft, synthesis window, overlap-add in frame order, crop."""
    rt = _real(precision)
    T = X.shape[0]
    X = np.asarray(X, np.complex64 if precision == "f32" else np.complex128)
    fr = scipy.fft.irfft(X, n=FFT, axis=1).astype(rt) * synthesis_window().astype(rt)
    out = np.zeros(HOP * (T - 1) + FFT, rt)
    for t in range(T):
        out[HOP * t:HOP * t + FFT] += fr[t]
    out = out[FADE:len(out) - FADE]
    if len(out) >= n:
        return out[:n]
    return np.concatenate([out, np.zeros(n - len(out), rt)])


def delayed(y, taps: int, delay: int):
    """y [F][T] -> ytilde [F][K][T]: ytilde[:, k, t] = y[:, t - delay - k], zeros before 0."""
    F, T = y.shape
    yt = np.zeros((F, taps, T), y.dtype)
    for k in range(taps):
        d = delay + k
        if d < T:
            yt[:, k, d:] = y[:, :T - d]
    return yt


def solve_bin(R, p):
    """g = R^-1 p by Cholesky with the contract's pivot rule: a pivot that is not > 1e-12 times
    the largest diagonal entry of R removes the tap (coefficient 0, row and column dropped)."""
    K = R.shape[0]
    L = np.zeros((K, K), np.complex128)
    diag = np.zeros(K)
    tol = 1e-12 * max(float(np.max(R.diagonal().real)), 0.0)
    for j in range(K):
        d = R[j, j].real - np.sum(np.abs(L[j, :j]) ** 2)
        if not d > tol:
            continue
        diag[j] = np.sqrt(d)
        for i in range(j + 1, K):
            L[i, j] = (R[i, j] - np.sum(L[i, :j] * np.conj(L[j, :j]))) / diag[j]
    z = np.zeros(K, np.complex128)
    for j in range(K):
        if diag[j] > 0:
            z[j] = (p[j] - np.sum(L[j, :j] * z[:j])) / diag[j]
    g = np.zeros(K, np.complex128)
    for j in range(K - 1, -1, -1):
        if diag[j] > 0:
            g[j] = (z[j] - np.sum(np.conj(L[j + 1:, j]) * g[j + 1:])) / diag[j]
    return g


def predict(y, yt, g, precision="f64"):
    """x = y - g^H ytilde; y [F][T], yt [F][K][T], g [F][K]."""
    if precision == "f32":
        g = g.astype(np.complex64)
    return y - np.einsum("fk,fkt->ft", np.conj(g), yt)


def correlations(y, yt, x, max_sq, precision="f64"):
    """R [F][K][K] and p [F][K] (complex128) of one iteration from the current estimate x and the
    chunk's max |x|^2: lambda = max(|x|^2, 1e-10 max_sq), in float32 with precision="f32"."""
    rt = _real(precision)
    eps = rt(1e-10) * rt(max_sq)
    lam = np.maximum((x.real.astype(rt) ** 2 + x.imag.astype(rt) ** 2), eps).astype(np.float64)
    inv = np.where(lam > 0, 1.0 / np.where(lam > 0, lam, 1.0), 0.0)
    y64, yt64 = y.astype(np.complex128), yt.astype(np.complex128)
    R = np.einsum("fit,fjt,ft->fij", yt64, np.conj(yt64), inv)
    p = np.einsum("fit,ft,ft->fi", yt64, np.conj(y64), inv)
    return R, p


def cond_of(R):
    """cond_2 of every R [F][K][K]: inf for a singular one, 0 for an all-zero one."""
    sv = np.linalg.svd(R, compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sv[:, 0] > 0, sv[:, 0] / sv[:, -1], 0.0)


def iteration(y, yt, x, max_sq, precision="f64"):
    """One WPE iteration on y [F][T] from the current estimate x and the chunk's max |x|^2:
    (g [F][K] complex128, the largest cond(R) over the bins)."""
    R, p = correlations(y, yt, x, max_sq, precision)
    g = np.stack([solve_bin(R[f], p[f]) for f in range(R.shape[0])])
    return g, float(np.max(cond_of(R)))


def wpe(Y, taps=10, delay=3, iterations=3, precision="f64", info=None):
    """Y [T][257] -> X [T][257].  info (a dict) receives "g" per iteration, "max_sq" per
    iteration and "cond", the largest cond(R) over bins and iterations."""
    y = np.ascontiguousarray(Y.T)
    yt = delayed(y, taps, delay)
    x = y
    cond = 0.0
    gs, maxes = [], []
    for _ in range(iterations):
        max_sq = float(np.max(np.abs(x) ** 2)) if x.size else 0.0
        maxes.append(max_sq)
        if not max_sq > 0:
            break
        g, c = iteration(y, yt, x, max_sq, precision)
        cond = max(cond, c)
        gs.append(g)
        x = predict(y, yt, g, precision)
    if info is not None:
        info.update(g=gs, max_sq=maxes, cond=cond)
    return np.ascontiguousarray(x.T)


def apply_wpe(audio, taps=10, delay=3, iterations=3, precision="f64", info=None):
    """The whole contract on one chunk: float64 output, float32 with precision="f32"."""
    audio = np.asarray(audio)
    n = len(audio)
    if n < 2 * FFT:
        return audio
    Y = stft(audio, precision)
    X = wpe(Y, taps, delay, iterations, precision, info)
    out = istft(X, n, precision)
    return out.astype(np.float32) if precision == "f32" else out


# ---- the parity inputs (shared by the CPU conditioning check and the GPU tests) -------------

def reverberant_speech(n: int, seed: int = 0, peak: float = 0.8):
    """Synthetic harmonic speech (syllables of a gliding fundamental with a few harmonics, short
    pauses, a little noise) through a 0.6 s exponential-decay room response, peak `peak`."""
    rng = np.random.default_rng(seed)
    sr = 16000
    t = np.arange(n) / sr
    dry = np.zeros(n)
    pos = 0
    while pos < n:
        dur = int(rng.uniform(0.08, 0.3) * sr)
        end = min(n, pos + dur)
        f0 = rng.uniform(90, 220) * (1 + 0.1 * np.sin(2 * np.pi * rng.uniform(2, 5) * t[pos:end]))
        ph = 2 * np.pi * np.cumsum(f0) / sr
        seg = sum(rng.uniform(0.2, 1.0) / h * np.sin(h * ph + rng.uniform(0, 6.28))
                  for h in range(1, 24))
        seg *= np.hanning(end - pos)
        dry[pos:end] += seg
        pos = end + int(rng.uniform(0.0, 0.08) * sr)
    dry += 0.02 * rng.standard_normal(n)
    L = int(0.6 * sr)
    h = rng.standard_normal(L) * np.exp(-6.9 * np.arange(L) / L)
    h[0] = 1.0
    wet = scipy.signal.fftconvolve(dry, h)[:n]
    return (wet * (peak / np.max(np.abs(wet)))).astype(np.float32)
