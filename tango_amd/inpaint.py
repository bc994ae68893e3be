"""Host-side helpers of masked-latent audio inpainting (AudioLDM's `super_resolution_and_inpainting`, audioldm/pipeline.py:249-301 ->
`generate_sample_masked`, audioldm/ldm.py:724-818): the latent mask and the waveform preparation in front of the mel front-end.
The loop itself is the engine's (Engine.denoise with `known_latents` / `latent_mask`, AudioDiffusion.inpaint, Tango.inpaint)."""
import numpy as np
import torch

#: hop size of the mel front-end and the number of frames a clip is cut or padded to (tools/torch_tools.py:66-68)
HOP = 160
TARGET_FRAMES = 1024
SEGMENT = TARGET_FRAMES * HOP

#: the clip lengths the engine generates, edits and inpaints: multiples of 2.5 s (the grid of audioldm/pipeline.py:49-50) up to the
#: 20 s the reference names as its ceiling (pipeline.py:168-170); 10 s is the default everywhere
DURATION_STEP, MAX_DURATION, DEFAULT_DURATION = 2.5, 20.0, 10.0
#: latent rows per grid step: int(2.5 * 25.6) (duration_to_latent_t_size, pipeline.py:94-95); the latent width is always 16
LATENT_ROWS_PER_STEP, LATENT_W = 64, 16


def vocoder_samples(frames, hifigan=None):
    """samples HiFi-GAN makes of `frames` mel frames: every ConvTranspose1d maps L to (L - 1) u - 2 ((k - u) // 2) + k
    (tango_engine_vocoder_samples; 160 * frames + 32 with the 16 kHz configuration)"""
    if hifigan is None:
        from .engine import HIFIGAN_CONFIG as hifigan
    n = int(frames)
    for u, k in zip(hifigan["upsample_rates"], hifigan["upsample_kernel_sizes"]):
        n = (n - 1) * u - 2 * ((k - u) // 2) + k
    return n


def duration_geometry(duration):
    """`duration` in seconds -> (latent height H = int(duration * 25.6), mel frames 4 H, waveform samples vocoder_samples(4 H)).
    Only the grid 2.5, 5, ..., 20 s is supported; anything else is a ValueError naming the grid values on either side (nothing is
    rounded silently)."""
    try:
        d = float(duration)
    except (TypeError, ValueError):
        raise ValueError("duration must be a number of seconds, got %r" % (duration,))
    k = d / DURATION_STEP
    nmax = int(MAX_DURATION / DURATION_STEP)
    if not (1 <= k <= nmax and k == int(k)):          # (NaN compares false)
        lo = (int(min(max(k, 1), nmax - 1)) if d == d else 1) * DURATION_STEP
        raise ValueError("duration %r s is not on the %g s grid up to %g s: the neighbouring durations are %g and %g"
                         % (duration, DURATION_STEP, MAX_DURATION, lo, lo + DURATION_STEP))
    h = LATENT_ROWS_PER_STEP * int(k)
    return h, 4 * h, vocoder_samples(4 * h)


def check_latent_h(h):
    """the latent heights of the duration grid (64, 128, ..., 512): a ValueError for any other"""
    nmax = int(MAX_DURATION / DURATION_STEP)
    if int(h) != h or h % LATENT_ROWS_PER_STEP or not 1 <= h // LATENT_ROWS_PER_STEP <= nmax:
        lo = min(max(int(h) // LATENT_ROWS_PER_STEP, 1), nmax - 1) * LATENT_ROWS_PER_STEP
        raise ValueError("latent height %r is not one of %d, %d, ..., %d (durations of 2.5 .. 20 s): the neighbouring heights are %d and %d"
                         % (h, LATENT_ROWS_PER_STEP, 2 * LATENT_ROWS_PER_STEP, nmax * LATENT_ROWS_PER_STEP, lo, lo + LATENT_ROWS_PER_STEP))
    return int(h)


#: latent rows per second (duration_to_latent_t_size, pipeline.py:94-95) and the most windows one long clip is cut into (the engine's limit)
LATENT_ROWS_PER_SECOND, MAX_WINDOWS = 25.6, 32


def long_geometry(duration, window=10.0, hop=5.0):
    """A clip longer than `window` seconds as overlapping windows in time (MultiDiffusion; the fork's panorama get_views,
    pipeline_stable_diffusion_panorama.py:442-456): `duration` s -> (H, Hw, s, V) in latent rows, the canvas height
    H = int(duration * 25.6), the window height Hw = duration_geometry(window)[0], the stride s = hop * 25.6 -- an integer multiple
    of 8 no larger than Hw -- and V = (H - Hw) / s + 1 <= 32 views.  The views must cover the canvas exactly, (H - Hw) % s == 0 (the
    fork floors and leaves a tail no view covers): otherwise a ValueError names the nearest valid durations on both sides."""
    try:
        d, hp = float(duration), float(hop)
    except (TypeError, ValueError):
        raise ValueError("duration and hop must be numbers of seconds, got %r and %r" % (duration, hop))
    hw = duration_geometry(window)[0]
    s = hp * LATENT_ROWS_PER_SECOND
    if not (s == int(s) and int(s) >= 8 and int(s) % 8 == 0):       # (NaN compares false)
        raise ValueError("hop %r s is %r latent rows: the stride must be an integer multiple of 8 rows (0.3125 s)" % (hop, s))
    s = int(s)
    if s > hw:
        raise ValueError("hop %r s exceeds the window of %r s: the windows would leave gaps" % (hop, window))
    if not d > float(window):
        raise ValueError("duration %r s does not exceed the window of %r s: generate() serves it" % (duration, window))
    if not d * LATENT_ROWS_PER_SECOND < 2 ** 31:                    # (NaN and inf end here)
        raise ValueError("duration %r s is not a clip length" % (duration,))
    h = int(d * LATENT_ROWS_PER_SECOND + 1e-6)                      # (25.6 is no binary fraction: 1e-6 rows absorb the product's rounding)
    k = (h - hw) // s
    if (h - hw) % s or abs(d * LATENT_ROWS_PER_SECOND - h) > 1e-6:  # a fraction of a row is not rounded away silently
        kk = min(max(k, 1), MAX_WINDOWS - 2)                         # at either end of the range: the two durations next to it
        lo, hi = (hw + kk * s) / LATENT_ROWS_PER_SECOND, (hw + (kk + 1) * s) / LATENT_ROWS_PER_SECOND
        raise ValueError("duration %r s is not window + k * hop (%r s + k * %r s): the neighbouring durations are %g and %g"
                         % (duration, window, hop, lo, hi))
    v = k + 1
    if v > MAX_WINDOWS:
        raise ValueError("duration %r s needs %d windows of %r s every %r s: at most %d (%g s)"
                         % (duration, v, window, hop, MAX_WINDOWS, (hw + (MAX_WINDOWS - 1) * s) / LATENT_ROWS_PER_SECOND))
    return h, hw, s, v


def loop_geometry(duration, window=None, hop=None):
    """A seamless loop of `duration` seconds as windows on a ring in time: -> (H, Hw, s, V) in latent rows, the ring's height
    H = duration * 25.6, the window height Hw = duration_geometry(window)[0] <= H, the stride s = hop * 25.6 -- an integer multiple
    of 8 rows below Hw that divides H -- and V = H / s <= 32 views, view v covering ring rows (v s + y) mod H (common.h window_cover).
    `window` defaults to `duration` when that is a length of generate()'s grid of at most 10 s, else to 10 s; `hop` to window / 2.
    A duration that is no whole number of strides is a ValueError naming the nearest valid durations on both sides."""
    try:
        d = float(duration)
    except (TypeError, ValueError):
        raise ValueError("duration must be a number of seconds, got %r" % (duration,))
    if not abs(d) * LATENT_ROWS_PER_SECOND < 2 ** 31:              # (NaN and inf end here)
        raise ValueError("duration %r s is not a clip length" % (duration,))
    if window is None:
        k = d / DURATION_STEP
        window = d if (k == int(k) and 1 <= k <= DEFAULT_DURATION / DURATION_STEP) else DEFAULT_DURATION
    hw = duration_geometry(window)[0]
    if hop is None:
        hop = float(window) / 2
    try:
        hp = float(hop)
    except (TypeError, ValueError):
        raise ValueError("hop must be a number of seconds, got %r" % (hop,))
    s = hp * LATENT_ROWS_PER_SECOND
    if not (s == int(s) and int(s) >= 8 and int(s) % 8 == 0):       # (NaN compares false)
        raise ValueError("hop %r s is %r latent rows: the stride must be an integer multiple of 8 rows (0.3125 s)" % (hop, s))
    s = int(s)
    if s >= hw:
        raise ValueError("hop %r s is not below the window of %r s: a loop needs overlapping windows" % (hop, window))
    if d < float(window):
        raise ValueError("duration %r s is shorter than the window of %r s: a window must not meet itself on the ring" % (duration, window))
    h = int(d * LATENT_ROWS_PER_SECOND + 1e-6)                      # (25.6 is no binary fraction: 1e-6 rows absorb the product's rounding)
    if h % s or abs(d * LATENT_ROWS_PER_SECOND - h) > 1e-6:         # a fraction of a row is not rounded away silently
        k = min(max(h // s, -(-hw // s)), MAX_WINDOWS - 1)           # at either end of the range: the two durations next to it
        lo, hi = k * s / LATENT_ROWS_PER_SECOND, (k + 1) * s / LATENT_ROWS_PER_SECOND
        raise ValueError("duration %r s is not a whole number of hops of %r s: the neighbouring durations are %g and %g"
                         % (duration, hop, lo, hi))
    v = h // s
    if v > MAX_WINDOWS:
        raise ValueError("duration %r s needs %d windows of %r s every %r s: at most %d (%g s)"
                         % (duration, v, window, hop, MAX_WINDOWS, MAX_WINDOWS * s / LATENT_ROWS_PER_SECOND))
    return h, hw, s, v


def window_taper(window_h, stride):
    """The weight of a window's local row y in the weighted update of timed prompts (include/tango_engine.h
    tango_engine_denoise_windows_weighted): np.float32 [window_h], with E = window_h - stride
        w[y] = min(1, (y + 0.5) / E) * min(1, (window_h - y - 0.5) / E)        (all ones when E == 0)
    computed in fp32 in mel_ring_blend_kernel's order of operations: a view fades in over its overlap with its predecessor and out
    over the one with its successor.  Every weight is strictly positive."""
    hw, s = int(window_h), int(stride)
    if hw != window_h or s != stride or hw < 1 or not 1 <= s <= hw:
        raise ValueError("window_taper takes integers 1 <= stride <= window_h, got window_h %r and stride %r" % (window_h, stride))
    e = hw - s
    if e == 0:
        return np.ones(hw, dtype=np.float32)
    y = np.arange(hw, dtype=np.float32)
    one, ef = np.float32(1.0), np.float32(e)
    up = np.minimum(one, (y + np.float32(0.5)) / ef)
    down = np.minimum(one, ((np.float32(hw) - y) - np.float32(0.5)) / ef)
    return (up * down).astype(np.float32)


def timeline_geometry(segments, duration, window=10.0, hop=5.0, loop=False):
    """Timed prompts: `segments` = [(prompt, start_seconds), ...] with ascending starts, the first at 0, on a clip of `duration` seconds
    cut into windows as long_geometry (loop False) or loop_geometry (loop True) cuts it.  Segment i starts at canvas row
    int(round(start_i * 25.6)) and ends where the next one starts (the last at H); window v runs under the prompt of the segment that
    holds its centre row v * s + Hw // 2 (mod H on a ring).  -> (H, Hw, s, V, window_prompt) with window_prompt the list of V segment
    indices.  Unsorted starts, a first start other than 0, a start at or beyond the duration and a segment that holds no window
    centre are ValueErrors that name the numbers."""
    H, hw, s, V = loop_geometry(duration, window, hop) if loop else long_geometry(duration, window, hop)
    try:
        starts = [float(st) for _, st in segments]
    except (TypeError, ValueError):
        raise ValueError("segments must be a list of (prompt, start_seconds) pairs, got %r" % (segments,))
    if not starts:
        raise ValueError("segments must hold at least one (prompt, start_seconds) pair")
    if starts[0] != 0.0:
        raise ValueError("the first segment must start at 0 s, got %r s" % (segments[0][1],))
    for i in range(1, len(starts)):
        if not starts[i] > starts[i - 1]:                            # (NaN compares false)
            raise ValueError("segment starts must ascend: segment %d starts at %r s, segment %d at %r s"
                             % (i - 1, segments[i - 1][1], i, segments[i][1]))
    for i, st in enumerate(starts):
        if not st < float(duration):
            raise ValueError("segment %d starts at %r s, at or beyond the duration of %r s" % (i, segments[i][1], duration))
    rows = [int(round(st * LATENT_ROWS_PER_SECOND)) for st in starts]
    centres = [(v * s + hw // 2) % H if loop else v * s + hw // 2 for v in range(V)]
    window_prompt = [max(i for i, r in enumerate(rows) if r <= c) for c in centres]
    for i, r in enumerate(rows):
        if i not in window_prompt:
            end = rows[i + 1] if i + 1 < len(rows) else H
            near = min(centres, key=lambda c: (abs(c - r), c))
            raise ValueError("segment %d (rows %d to %d, %g s to %g s) holds no window centre: the %d centres are every %g s from %g s; "
                             "the nearest is at %g s (row %d) -- start the segment there, or move its neighbour past it"
                             % (i, r, end, r / LATENT_ROWS_PER_SECOND, end / LATENT_ROWS_PER_SECOND, V, s / LATENT_ROWS_PER_SECOND,
                                min(centres) / LATENT_ROWS_PER_SECOND, near / LATENT_ROWS_PER_SECOND, near))
    return H, hw, s, V, window_prompt


def clip_duration(n_samples):
    """the smallest grid duration whose mel frames hold a 16 kHz clip of `n_samples` samples; 20 s for anything longer (the clip is
    then cut).  Unlike the reference's round_up_duration (pipeline.py:49-50), which always adds one more 2.5 s block -- a 5 s clip
    becomes 7.5 s --, a clip that fills a grid length exactly keeps it."""
    block = 4 * LATENT_ROWS_PER_STEP * HOP
    k = (max(int(n_samples), 1) + block - 1) // block
    return min(k * DURATION_STEP, MAX_DURATION)


def latent_mask(batch, time_range=(0.10, 0.15), freq_range=(1.0, 1.0), h=256, w=16):
    """[batch, 1, h, w] fp32 mask as ldm.py:773-777 builds it: ones, rows int(h * t0):int(h * t1) (time) and columns
    int(w * f0):int(w * f1) (mel frequency) zeroed.  1 keeps the known audio, 0 regenerates it.  The defaults are
    pipeline.py:259-262's: a time span of 10 % .. 15 % and an empty frequency span."""
    m = torch.ones(batch, h, w)
    m[:, int(h * time_range[0]):int(h * time_range[1]), :] = 0
    m[:, :, int(w * freq_range[0]):int(w * freq_range[1])] = 0
    return m[:, None, ...]


def prepare_waveform(audio, segment_length=SEGMENT, duration=DEFAULT_DURATION):
    """tools/torch_tools.py:9-54 after the resample: a 1-D 16 kHz clip -> fp32 [segment_length] = normalize_wav (remove the mean,
    divide by max |x| + 1e-8, halve), crop or zero-pad to `segment_length` samples, divide by max |x|, halve.  Reading the file and
    resampling stay with the caller.  `duration` (seconds on the 2.5 s grid) other than the default sets `segment_length` to that
    duration's mel frames times the hop; None takes clip_duration() of the clip: the clip is zero-padded up to the smallest grid
    duration that holds it and cut at 20 s."""
    x = torch.as_tensor(np.asarray(audio) if not torch.is_tensor(audio) else audio).to(torch.float32).cpu()
    if x.dim() != 1:
        raise ValueError("prepare_waveform takes one 1-D clip, got shape %s" % (tuple(x.shape),))
    if duration is None:
        duration = clip_duration(len(x))
    if duration != DEFAULT_DURATION:
        if segment_length != SEGMENT:
            raise ValueError("prepare_waveform takes a segment_length or a duration, not both")
        segment_length = duration_geometry(duration)[1] * HOP
    x = x - torch.mean(x)                                       # normalize_wav
    x = x / (torch.max(torch.abs(x)) + 1e-8)
    x = x * 0.5
    n = len(x)                                                  # pad_wav
    if n > segment_length:
        x = x[:segment_length]
    elif n < segment_length:
        x = torch.cat([x, torch.zeros(segment_length - n)])
    x = x / torch.max(torch.abs(x))
    return 0.5 * x
