"""The beat track, restated in numpy float64 from the definitions in include/tcdiff_hip.h (librosa 0.9.2's beat.beat_track,
beat.tempo and beat.__beat_tracker for one onset envelope at 60 frames / s): the yardstick of tests/test_beat_gpu.py.  Only numpy;
the sums whose order the definitions fix are explicit loops over taps.  Every decision the tracker makes (an argmax, a threshold,
a flag) is returned with its margin, so that a test can require the margins to exceed the kernel's rounding error before it asks
for equal decisions.

librosa is not installed where this project is built, so parity with librosa's own output is NOT pinned by anything here."""
import numpy as np

WIN = 480                                                 # the tempo estimate's window, 8 s
TINY = float(np.finfo(np.float32).tiny)


def make_envelope(T, every, seed):
    """T float32 frames: a 0.05 u noise floor, clicks of height 1 + 0.3 u every ``every`` frames from frame 7 (none if ``every`` is
    None), the first three frames zero as onset_env has them"""
    rng = np.random.default_rng(seed)
    o = 0.05 * rng.random(T)
    if every:
        at = np.arange(7, T, every)
        o[at] += 1.0 + 0.3 * rng.random(len(at))
    o[:3] = 0.0
    return o.astype(np.float32)


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _top_two_gap(v):
    """the largest value's distance to the second largest (inf with fewer than two finite values)"""
    f = np.sort(v[np.isfinite(v)])
    return float(f[-1] - f[-2]) if len(f) >= 2 else np.inf


# ---- tempo ------------------------------------------------------------------------------------------------------------------------
def tempo_prior(start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    with np.errstate(divide="ignore"):
        bpms = 3600.0 / np.arange(WIN)
    prior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / std_bpm) ** 2
    prior[bpms >= max_tempo] = -np.inf
    return prior


def mean_autocorrelation(o):
    """g[l]: the mean over the frames t of the normalised autocorrelation of padded samples [t, t + 480) times the window"""
    o = np.asarray(o, np.float64)
    T = len(o)
    pad = np.pad(o, WIN // 2, mode="linear_ramp", end_values=0.0)
    X = np.lib.stride_tricks.sliding_window_view(pad, WIN)[:T] * hann(WIN)
    A = np.empty((T, WIN))
    for lag in range(WIN):
        A[:, lag] = np.sum(X[:, :WIN - lag] * X[:, lag:], axis=1)
    mx = np.abs(A).max(axis=1, keepdims=True)
    A = np.where(mx < TINY, A, A / np.where(mx < TINY, 1.0, mx))
    g = np.zeros(WIN)
    for t in range(T):                                    # ascending t
        g += A[t]
    return g / T


def tempo(o, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """-> (tempo in beats per minute, lag, the score's top-two gap)"""
    score = np.log1p(1e6 * mean_autocorrelation(o)) + tempo_prior(start_bpm, std_bpm, max_tempo)
    lag = int(np.argmax(score))
    return 3600.0 / lag, lag, _top_two_gap(score)


# ---- local score --------------------------------------------------------------------------------------------------------------------
def local_score(o, period):
    o = np.asarray(o, np.float64)
    T = len(o)
    x = o / o.std(ddof=1)
    w = np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2)
    ls = np.zeros(T)
    for j in range(-period, period + 1):                  # ascending j: ls[i] += w[j] x[i - j]
        lo, hi = max(0, j), min(T, T + j)                 # 0 <= i - j < T
        if lo < hi:
            ls[lo:hi] = ls[lo:hi] + w[j + period] * x[lo - j:hi - j]
    return ls


# ---- dynamic programme ----------------------------------------------------------------------------------------------------------------
def half_period(period):
    return int(np.round(period / 2))                      # half to even


def transition(period, tightness):
    d = np.arange(-2 * period, -half_period(period) + 1)
    with np.errstate(divide="ignore"):
        return d, -tightness * (np.log(-d / period) ** 2)


def programme(ls, period, tightness, block=1):
    """-> cum, back, the smallest top-two gap of a frame's argmax, |ls - 0.01 max| over the frames that decide the first beat.
    ``block`` > 1 runs the frames in blocks that read a snapshot of cum taken at the block's start."""
    T = len(ls)
    d, txwt = transition(period, tightness)
    cum, back = np.zeros(T), np.zeros(T, np.int64)
    thr = 0.01 * ls.max()
    above = np.nonzero(ls >= thr)[0]
    first = int(above[0]) if len(above) else T
    gap = np.inf
    for i0 in range(0, T, block):
        snap = cum.copy() if block > 1 else cum
        for i in range(i0, min(T, i0 + block)):
            at = i + d
            c = txwt + np.where(at >= 0, snap[np.clip(at, 0, T - 1)], 0.0)
            k = int(np.argmax(c))
            gap = min(gap, _top_two_gap(c))
            cum[i] = ls[i] + c[k]
            back[i] = -1 if i < first else at[k]
    thr_margin = float(np.abs(ls[:min(first + 1, T)] - thr).min())
    return cum, back, gap, thr_margin


# ---- last beat, backtrace, trim ---------------------------------------------------------------------------------------------------------
def last_beat(cum):
    """-> (last or -1, flags, the smallest |cum[i] - cum[i +- 1]|, the smallest |2 cum - med| over the flagged frames)"""
    pad = np.pad(cum, 1, mode="edge")
    m = (cum > pad[:-2]) & (cum >= pad[2:])
    flag_margin = float(np.abs(np.diff(cum)).min())
    if not m.any():
        return -1, m, flag_margin, np.inf
    med = float(np.median(cum[m]))
    ok = m & (2.0 * cum > med)
    med_margin = float(np.abs(2.0 * cum[m] - med).min())
    return (int(np.nonzero(ok)[0].max()) if ok.any() else -1), m, flag_margin, med_margin


def backtrace(back, last):
    beats = []
    while last >= 0:
        beats.append(last)
        last = int(back[last])
    return np.array(beats[::-1], np.int64)


def trim_beats(ls, beats, trim):
    """-> (the kept beats, the smallest |s - thr|)"""
    n = len(beats)
    if n == 0:
        return beats, np.inf
    v = ls[beats]
    s = v.copy()
    s[1:] = 0.5 * v[:-1] + s[1:]
    s[:-1] = s[:-1] + 0.5 * v[1:]
    thr = 0.5 * np.sqrt(np.mean(s ** 2)) if trim else 0.0
    ok = np.nonzero(s > thr)[0]
    margin = float(np.abs(s - thr).min())
    if len(ok) == 0:
        return beats[:0], margin
    return beats[ok.min():ok.max()], margin                 # the end is exclusive


def beat_track(o, bpm=None, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, tightness=100.0, trim=True):
    """o (T,) float32 -> dict: tempo, period, local_score, cum_score, backlink, beats (the kept ones), n_beats, onset_beat and
    ``margins``: tempo (the score's top-two gap; absent with ``bpm``), argmax, first, flag, median, trim."""
    o = np.asarray(o, np.float32)
    T = len(o)
    out = dict(tempo=0.0, period=0, local_score=np.zeros(T), cum_score=np.zeros(T), backlink=np.full(T, -1, np.int64),
               beats=np.zeros(0, np.int64), n_beats=0, onset_beat=np.zeros(T, np.float32), margins={})
    if not o.any():
        if bpm is not None:
            out["period"] = int(np.round(3600.0 / bpm))
        return out
    if bpm is None:
        out["tempo"], out["period"], out["margins"]["tempo"] = tempo(o, start_bpm, std_bpm, max_tempo)
    else:
        out["tempo"], out["period"] = float(bpm), int(np.round(3600.0 / bpm))
    period = out["period"]
    if o.max() == o.min():                                # zero variance: no beats rather than NaNs
        return out
    ls = local_score(o, period)
    cum, back, gap, first_margin = programme(ls, period, tightness)
    last, _, flag_margin, med_margin = last_beat(cum)
    beats, trim_margin = trim_beats(ls, backtrace(back, last), trim)
    out.update(local_score=ls, cum_score=cum, backlink=back, beats=beats, n_beats=len(beats))
    out["onset_beat"][beats] = 1.0
    out["margins"].update(argmax=gap, first=first_margin, flag=flag_margin, median=med_margin, trim=trim_margin)
    return out


# ---- the cases of tests/test_beat_gpu.py, whose margin condition tests/test_beat_cpu.py checks before any GPU run -----------------------
# name -> T, clicks every, bpm given, seed.  The seeds of C and G are picked so that the flag margin (set by the near-equal
# cumulative scores of the first, silent frames at this short period) meets the condition.
CASES = {"A": (5, None, 120.0, 0), "B": (40, 30, 120.0, 0), "C": (64, 12, 300.0, 1), "D": (451, 30, None, 0),
         "E": (600, 27, None, 0), "F": (1000, 25, None, 0), "G": (700, 12, 300.0, 1)}
BOUND, MARGIN, TEMPO_GAP = 1e-12, 1e-10, 1e-3             # max |kernel - ref| / max |ref|; margins / max |cum|; the tempo score's gap
_cache = {}


def case(name, trim=True):
    """(envelope, reference) of a case, computed once and left unchanged"""
    key = (name, trim)
    if key not in _cache:
        T, every, bpm, seed = CASES[name]
        o = make_envelope(T, every, seed)
        _cache[key] = (o, beat_track(o, bpm=bpm, trim=trim))
    return _cache[key]


def batch_rows():
    """D's clip padded with the noise floor to E's length (silence would tie the programme's candidates exactly), a silent clip,
    E's clip: three rows of one T with two different periods"""
    if "batch" not in _cache:
        d, e = case("D")[0], case("E")[0]
        floor = (0.05 * np.random.default_rng(7).random(len(e) - len(d))).astype(np.float32)
        rows = [np.concatenate([d, floor]), np.zeros(len(e), np.float32), e]
        _cache["batch"] = (rows, [beat_track(o) for o in rows])
    return _cache["batch"]


def margin_failures(ref):
    """the decision margins of a reference run that miss the condition under which the kernel must decide as the reference does"""
    scale = float(np.abs(ref["cum_score"]).max())
    bad = [(k, v, MARGIN * scale) for k, v in ref["margins"].items() if k != "tempo" and not v >= MARGIN * scale]
    if "tempo" in ref["margins"] and not ref["margins"]["tempo"] >= TEMPO_GAP:
        bad.append(("tempo", ref["margins"]["tempo"], TEMPO_GAP))
    return bad
