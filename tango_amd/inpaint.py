"""Host-side helpers of masked-latent audio inpainting (AudioLDM's `super_resolution_and_inpainting`, audioldm/pipeline.py:249-301 ->
`generate_sample_masked`, audioldm/ldm.py:724-818): the latent mask and the waveform preparation in front of the mel front-end.
The loop itself is the engine's (Engine.denoise with `known_latents` / `latent_mask`, AudioDiffusion.inpaint, Tango.inpaint)."""
import numpy as np
import torch

#: hop size of the mel front-end and the number of frames a clip is cut or padded to (tools/torch_tools.py:66-68)
HOP = 160
TARGET_FRAMES = 1024
SEGMENT = TARGET_FRAMES * HOP


def latent_mask(batch, time_range=(0.10, 0.15), freq_range=(1.0, 1.0), h=256, w=16):
    """[batch, 1, h, w] fp32 mask as ldm.py:773-777 builds it: ones, rows int(h * t0):int(h * t1) (time) and columns
    int(w * f0):int(w * f1) (mel frequency) zeroed.  1 keeps the known audio, 0 regenerates it.  The defaults are
    pipeline.py:259-262's: a time span of 10 % .. 15 % and an empty frequency span."""
    m = torch.ones(batch, h, w)
    m[:, int(h * time_range[0]):int(h * time_range[1]), :] = 0
    m[:, :, int(w * freq_range[0]):int(w * freq_range[1])] = 0
    return m[:, None, ...]


def prepare_waveform(audio, segment_length=SEGMENT):
    """tools/torch_tools.py:9-54 after the resample: a 1-D 16 kHz clip -> fp32 [segment_length] = normalize_wav (remove the mean,
    divide by max |x| + 1e-8, halve), crop or zero-pad to `segment_length` samples, divide by max |x|, halve.  Reading the file and
    resampling stay with the caller."""
    x = torch.as_tensor(np.asarray(audio) if not torch.is_tensor(audio) else audio).to(torch.float32).cpu()
    if x.dim() != 1:
        raise ValueError("prepare_waveform takes one 1-D clip, got shape %s" % (tuple(x.shape),))
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
