"""Host-side audio processing for Synthesizer.tts: the Griffin-Lim CPU fallback (config C1), silence
trimming and wav writing. Restates `TTS/utils/audio.py` (AudioProcessor) without librosa, which
is not in this image: the mel filterbank is librosa.filters.mel's published Slaney algorithm,
STFT/ISTFT are torch.stft/istft with librosa's conventions (periodic Hann, centred frames, the
config's pad mode), trimming is librosa.effects.trim's frame-RMS rule. Mean-var scaling (`stats_path`,
audio.py:80-86,108-186) reads compute_statistics.py's stats file through a restricted loader
(`load_stats_file`). By default none of these touch the GPU; the audio-config key
``griffin_lim_device: "gpu"`` moves `inv_melspectrogram` onto the library's batched Griffin-Lim
kernels (`inv_melspectrogram_batch`, fp32), ``analysis_device: "gpu"`` moves `spectrogram` /
`melspectrogram` onto its analysis kernels (`spectrogram_batch` / `melspectrogram_batch`, fp32), and
``wav_tail_device: "gpu"`` lets `Synthesizer` run de-emphasis and the end of `tts()` (endpoints, join,
16-bit scaling) on the device (`deemphasis_batch`, `finish_batch`); everything else stays on the host. Parity of the restated librosa pieces is unpinned
(librosa is not importable here to make fixtures); tests check their defining properties.
"""
import io
import json
import pickle

import numpy as np
import scipy.io.wavfile
import torch


def _hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False)."""
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * m
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), freqs)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with Slaney area normalisation."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


class StandardScaler:
    """tts/utils/data.py:56-76."""

    def set_stats(self, mean, scale):
        self.mean_ = mean
        self.scale_ = scale

    def reset_stats(self):
        delattr(self, "mean_")
        delattr(self, "scale_")

    def transform(self, X):
        X = np.asarray(X)
        X -= self.mean_
        X /= self.scale_
        return X

    def inverse_transform(self, X):
        X = np.asarray(X)
        X *= self.scale_
        X += self.mean_
        return X


class _StatsConfig(dict):
    """Stand-in for `TTS.utils.io.AttrDict`, the class compute_statistics.py pickles the audio
    config as: keys as attributes, nothing else."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def __setstate__(self, state):  # the pickled __dict__ is the dict itself (AttrDict)
        pass


class _StatsUnpickler(pickle.Unpickler):
    """Admits exactly what `np.save(path, stats_dict)` writes: numpy array / dtype / scalar
    reconstruction, builtin containers, and the reference's AttrDict (as a plain dict). Any other
    global in the stream is refused before anything from it runs (the same rule as
    torch.load(weights_only=True))."""

    _NUMPY = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
              ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
              ("numpy", "ndarray"), ("numpy", "dtype")}

    def find_class(self, module, name):
        if (module, name) in self._NUMPY:
            return super().find_class(module, name)
        if name == "AttrDict" and module in ("TTS.utils.io", "mozilla_voice_tts.utils.io"):
            return _StatsConfig
        raise pickle.UnpicklingError(f"stats file references {module}.{name}: refused")


def load_stats_file(path):
    """The mean-var stats dict (mel_mean, mel_std, linear_mean, linear_std, audio_config).
    `.npz`: plain arrays (audio_config as a JSON string), read with allow_pickle=False. `.npy`:
    the object array compute_statistics.py writes (`np.save(path, dict, allow_pickle=True)`),
    read through `_StatsUnpickler` instead of numpy's unrestricted pickle load."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            out = {k: z[k] for k in ("mel_mean", "mel_std", "linear_mean", "linear_std")}
            out["audio_config"] = json.loads(str(z["audio_config"]))
        return out
    with open(path, "rb") as f:
        version = np.lib.format.read_magic(f)
        read_header = (np.lib.format.read_array_header_1_0 if version == (1, 0)
                       else np.lib.format.read_array_header_2_0)
        _shape, _fortran, dtype = read_header(f)
        if not dtype.hasobject:
            raise ValueError(f"{path}: expected the pickled stats dict, found a plain {dtype} array")
        arr = _StatsUnpickler(f).load()
    stats = arr.item() if isinstance(arr, np.ndarray) else arr
    if not isinstance(stats, dict):
        raise ValueError(f"{path}: stats file does not hold a dict")
    return stats


class AudioProcessor:
    """The subset of TTS/utils/audio.py:11-345 that Synthesizer.tts uses."""

    def __init__(self, sample_rate=None, num_mels=None, min_level_db=None, frame_shift_ms=None,
                 frame_length_ms=None, hop_length=None, win_length=None, ref_level_db=None, fft_size=1024,
                 power=None, preemphasis=0.0, signal_norm=None, symmetric_norm=None, max_norm=None,
                 mel_fmin=None, mel_fmax=None, spec_gain=20, stft_pad_mode="reflect", clip_norm=True,
                 griffin_lim_iters=None, do_trim_silence=False, trim_db=60, stats_path=None, griffin_lim_device=None,
                 analysis_device=None, wav_tail_device=None, **_):
        if griffin_lim_device not in (None, "cpu", "gpu"):
            raise ValueError(f"griffin_lim_device must be 'cpu' or 'gpu', got {griffin_lim_device!r}")
        if analysis_device not in (None, "cpu", "gpu"):
            raise ValueError(f"analysis_device must be 'cpu' or 'gpu', got {analysis_device!r}")
        if wav_tail_device not in (None, "cpu", "gpu"):
            raise ValueError(f"wav_tail_device must be 'cpu' or 'gpu', got {wav_tail_device!r}")
        # None / "cpu": Griffin-Lim on the host (float64); "gpu": the library's batched kernels (fp32)
        self.griffin_lim_device = griffin_lim_device
        self._gl_dev_cache = {}
        # None / "cpu": spectrogram / melspectrogram on the host (float64); "gpu": the batched
        # analysis kernels at B = 1 (fp32)
        self.analysis_device = analysis_device
        self._an_dev_cache = {}
        # None / "cpu": Synthesizer de-emphasises, finds endpoints, joins and scales on the host;
        # "gpu": on the device (`deemphasis_batch`, `finish_batch`). The methods here ignore it.
        self.wav_tail_device = wav_tail_device
        self.sample_rate = sample_rate
        self.num_mels = num_mels
        self.min_level_db = min_level_db or 0
        self.ref_level_db = ref_level_db
        self.fft_size = fft_size
        self.power = power
        self.preemphasis = preemphasis
        self.griffin_lim_iters = griffin_lim_iters
        self.signal_norm = signal_norm
        self.symmetric_norm = symmetric_norm
        self.max_norm = 1.0 if max_norm is None else float(max_norm)
        self.mel_fmin = mel_fmin or 0
        self.mel_fmax = mel_fmax
        self.spec_gain = float(spec_gain)
        self.stft_pad_mode = stft_pad_mode
        self.clip_norm = clip_norm
        self.do_trim_silence = do_trim_silence
        self.trim_db = trim_db
        self.frame_shift_ms, self.frame_length_ms = frame_shift_ms, frame_length_ms
        self.do_sound_norm = _.get("do_sound_norm", False)
        self.stats_path = stats_path
        if hop_length is None:  # audio.py:99-105
            factor = frame_length_ms / frame_shift_ms
            assert float(factor).is_integer(), " [!] frame_shift_ms should divide frame_length_ms"
            hop_length = int(frame_shift_ms / 1000.0 * sample_rate)
            win_length = int(hop_length * factor)
        self.hop_length, self.win_length = hop_length, win_length
        assert self.min_level_db != 0.0, " [!] min_level_db is 0"
        assert self.win_length <= self.fft_size, " [!] win_length cannot be larger than fft_size"
        self.mel_basis = mel_filterbank(sample_rate, fft_size, num_mels, self.mel_fmin, self.mel_fmax)
        self.inv_mel_basis = np.linalg.pinv(self.mel_basis)
        if stats_path:  # audio.py:80-86: mean-var scaling replaces the range normalisation
            mel_mean, mel_std, linear_mean, linear_std, _cfg = self.load_stats(stats_path)
            self.setup_scaler(mel_mean, mel_std, linear_mean, linear_std)
            self.signal_norm = True
            self.max_norm = None
            self.clip_norm = None
            self.symmetric_norm = None

    # -- mean-var scaling (audio.py:165-186, tts/utils/data.py:56-76)
    def load_stats(self, stats_path):
        """audio.py:165-180: the stats file `TTS/bin/compute_statistics.py:59-80` writes, checked
        against this processor's parameters (the same skip list)."""
        stats = load_stats_file(stats_path)
        stats_config = stats["audio_config"]
        skip = ["griffin_lim_iters", "stats_path", "do_trim_silence", "ref_level_db", "power"]
        for key in stats_config.keys():
            if key in skip or key == "sample_rate":
                continue
            assert stats_config[key] == self.__dict__[key], \
                f" [!] Audio param {key} does not match the value used for computing mean-var stats. " \
                f"{stats_config[key]} vs {self.__dict__[key]}"
        return stats["mel_mean"], stats["mel_std"], stats["linear_mean"], stats["linear_std"], stats_config

    def setup_scaler(self, mel_mean, mel_std, linear_mean, linear_std):
        self.mel_scaler = StandardScaler()
        self.mel_scaler.set_stats(mel_mean, mel_std)
        self.linear_scaler = StandardScaler()
        self.linear_scaler.set_stats(linear_mean, linear_std)

    def _scaler_for(self, S):
        """audio.py:114-120 / 143-149: picked by the feature count. The linear branch compares
        with fft_size / 2 exactly as the reference does."""
        if S.shape[0] == self.num_mels:
            return self.mel_scaler
        if S.shape[0] == self.fft_size / 2:
            return self.linear_scaler
        raise RuntimeError(" [!] Mean-Var stats does not match the given feature dimensions.")

    # -- normalisation (audio.py:108-163)
    def _normalize(self, S):
        if not self.signal_norm:
            return S.copy()
        if hasattr(self, "mel_scaler"):
            return self._scaler_for(S).transform(S.copy().T).T
        S = S - self.ref_level_db
        S_norm = (S - self.min_level_db) / (-self.min_level_db)
        if self.symmetric_norm:
            S_norm = (2 * self.max_norm) * S_norm - self.max_norm
            return np.clip(S_norm, -self.max_norm, self.max_norm) if self.clip_norm else S_norm
        S_norm = self.max_norm * S_norm
        return np.clip(S_norm, 0, self.max_norm) if self.clip_norm else S_norm

    def _denormalize(self, S):
        S = S.copy()
        if not self.signal_norm:
            return S
        if hasattr(self, "mel_scaler"):
            return self._scaler_for(S).inverse_transform(S.T).T
        if self.symmetric_norm:
            if self.clip_norm:
                S = np.clip(S, -self.max_norm, self.max_norm)
            S = (S + self.max_norm) * -self.min_level_db / (2 * self.max_norm) + self.min_level_db
            return S + self.ref_level_db
        if self.clip_norm:
            S = np.clip(S, 0, self.max_norm)
        return S * -self.min_level_db / self.max_norm + self.min_level_db + self.ref_level_db

    def _amp_to_db(self, x):
        return self.spec_gain * np.log10(np.maximum(1e-5, x))

    def _db_to_amp(self, x):
        return np.power(10.0, x / self.spec_gain)

    # -- STFT (audio.py:259-279), librosa conventions on torch
    def _window(self):
        return torch.hann_window(self.win_length, periodic=True, dtype=torch.float64)

    def _stft(self, y):
        t = torch.as_tensor(np.asarray(y, np.float64))
        D = torch.stft(t, self.fft_size, self.hop_length, self.win_length, self._window(), center=True,
                       pad_mode=self.stft_pad_mode, return_complex=True)
        return D.numpy()

    def _istft(self, D):
        t = torch.as_tensor(D)
        return torch.istft(t, self.fft_size, self.hop_length, self.win_length, self._window(), center=True).numpy()

    def _griffin_lim(self, S, rng=None):
        rng = np.random if rng is None else rng
        angles = np.exp(2j * np.pi * rng.rand(*S.shape))
        S_complex = np.abs(S).astype(np.complex128)
        y = self._istft(S_complex * angles)
        for _ in range(self.griffin_lim_iters):
            angles = np.exp(1j * np.angle(self._stft(y)))
            y = self._istft(S_complex * angles)
        return y

    def _preemph_stft(self, y):
        if self.preemphasis != 0:  # audio.py:198-202
            import scipy.signal
            y = scipy.signal.lfilter([1, -self.preemphasis], [1], y)
        return self._stft(y)

    def spectrogram(self, y):
        """audio.py:216-222. With ``analysis_device == "gpu"`` the batched GPU path runs at B = 1
        (fp32) and the (fft_size / 2 + 1, M) result comes back as numpy."""
        if self.analysis_device == "gpu":
            return self._analysis_single(y, mel=False)
        return self._normalize(self._amp_to_db(np.abs(self._preemph_stft(y))))

    def melspectrogram(self, y):
        """audio.py:224-230. With ``analysis_device == "gpu"``: as `spectrogram`, (num_mels, M)."""
        if self.analysis_device == "gpu":
            return self._analysis_single(y, mel=True)
        return self._normalize(self._amp_to_db(self.mel_basis @ np.abs(self._preemph_stft(y))))

    # -- batched analysis on the GPU (tts_stft_mag + tts_mag_to_feature)
    def _norm_affine(self, n_channels):
        """`_normalize` on a dB feature of ``n_channels`` rows as clip(dB * scale + offset) per
        channel: (scale, offset, clip) with clip None or the (lo, hi) bounds. The inverse of
        `_denorm_affine`; with mean-var stats the scaler is picked as `_scaler_for` picks it."""
        ones = np.ones(n_channels)
        if not self.signal_norm:
            return ones, 0.0 * ones, None
        if hasattr(self, "mel_scaler"):
            sc = self._scaler_for(np.empty((n_channels, 0)))
            std, mean = np.asarray(sc.scale_, np.float64), np.asarray(sc.mean_, np.float64)
            return 1.0 / std, -mean / std, None
        span = -self.min_level_db
        base = (-self.ref_level_db - self.min_level_db) / span
        if self.symmetric_norm:
            scale, offset = 2 * self.max_norm / span, 2 * self.max_norm * base - self.max_norm
            clip = (-self.max_norm, self.max_norm) if self.clip_norm else None
        else:
            scale, offset = self.max_norm / span, self.max_norm * base
            clip = (0.0, self.max_norm) if self.clip_norm else None
        return scale * ones, offset * ones, clip

    def _analysis_check_params(self):
        """What the GPU analysis covers (include/ttship.h, tts_stft_mag)."""
        if self.stft_pad_mode != "reflect":
            raise NotImplementedError(f"GPU analysis: stft_pad_mode={self.stft_pad_mode!r} (only 'reflect')")
        if self.fft_size % 2 or not 64 <= self.fft_size <= 2048:
            raise NotImplementedError(f"GPU analysis: fft_size={self.fft_size} (even, 64 to 2048)")
        if not 16 <= self.hop_length <= self.fft_size:
            raise NotImplementedError(f"GPU analysis: hop_length={self.hop_length} (16 to fft_size)")

    def _analysis_batch(self, wavs, lengths, mel):
        from ._lib import get_engine
        self._analysis_check_params()
        n_freq = self.fft_size // 2 + 1
        n_out = self.num_mels if mel else n_freq
        dev = wavs.device
        eng = get_engine(dev)
        key = (dev, mel)
        if key not in self._an_dev_cache:
            scale, offset, clip = self._norm_affine(n_out)
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
            self._an_dev_cache[key] = (put(self.mel_basis) if mel else None, put(scale), put(offset), clip)
        basis, scale, offset, clip = self._an_dev_cache[key]
        wavs = wavs.contiguous().float()
        B = wavs.shape[0]
        lengths = [int(n) for n in lengths]
        assert wavs.dim() == 2 and len(lengths) == B
        frames = [1 + n // self.hop_length for n in lengths]
        M = max(frames)
        mag = torch.empty(B, M, n_freq, device=dev)
        out = torch.empty(B, M, n_out, device=dev)
        with eng.lock:
            eng.stft_mag(wavs, lengths, self.fft_size, self.win_length, self.hop_length, self.preemphasis, mag)
            eng.mag_to_feature(mag, frames, basis, self.spec_gain, scale, offset, clip, out)
        return out, frames

    def spectrogram_batch(self, wavs, lengths):
        """`spectrogram` of a batch on the GPU: ``wavs`` (B, L_max) waveform rows on a ROCm device,
        row b valid for ``lengths[b]`` samples (more than fft_size / 2 each). Returns the
        (B, M_max, fft_size / 2 + 1) frame-major device tensor (rows zero past their own frame count)
        and the per-row frame counts 1 + lengths[b] // hop_length."""
        return self._analysis_batch(wavs, lengths, mel=False)

    def melspectrogram_batch(self, wavs, lengths):
        """`melspectrogram` of a batch on the GPU; as `spectrogram_batch`, (B, M_max, num_mels)."""
        return self._analysis_batch(wavs, lengths, mel=True)

    def _analysis_single(self, y, mel):
        y = np.ascontiguousarray(y, dtype=np.float32)
        out, frames = self._analysis_batch(torch.from_numpy(y[None]).cuda(), [y.shape[0]], mel)
        return np.ascontiguousarray(out[0, :frames[0]].cpu().numpy().T)

    def inv_melspectrogram(self, mel, rng=None):
        """audio.py:241-248 (no pre-emphasis path: raise as the reference would need scipy lfilter).
        With ``griffin_lim_device == "gpu"`` the batched GPU path runs at B = 1 (fp32; the phase is
        ``rng.rand(n_freq, M)`` when an ``rng`` is given) and the result comes back as numpy."""
        if self.griffin_lim_device == "gpu":
            mel = np.asarray(mel, np.float32)
            phase = None
            if rng is not None:
                u = np.asarray(rng.rand(self.fft_size // 2 + 1, mel.shape[1]), np.float32)
                phase = torch.from_numpy(np.ascontiguousarray(u.T)[None]).cuda()
            mels = torch.from_numpy(np.ascontiguousarray(mel.T)[None]).cuda()
            wav, _ = self.inv_melspectrogram_batch(mels, [mel.shape[1]], phase)
            wav = wav[0].cpu().numpy()
            if self.preemphasis != 0:
                import scipy.signal
                return scipy.signal.lfilter([1], [1, -self.preemphasis], wav)
            return wav
        S = self._db_to_amp(self._denormalize(mel))
        S = np.maximum(1e-10, self.inv_mel_basis @ S)
        if self.preemphasis != 0:
            import scipy.signal
            return scipy.signal.lfilter([1], [1, -self.preemphasis], self._griffin_lim(S ** self.power, rng))
        return self._griffin_lim(S ** self.power, rng)

    def inv_spectrogram(self, spectrogram, rng=None):
        """audio.py:232-239: a normalised linear spectrogram (fft_size / 2 + 1, M) -> waveform:
        denormalise, dB to amplitude, power, Griffin-Lim, inverse pre-emphasis if configured. With
        ``griffin_lim_device == "gpu"`` the phase reconstruction runs on the library's batched
        Griffin-Lim at B = 1 (fp32), behind the same parameter checks as the mel path."""
        S = self._db_to_amp(self._denormalize(np.asarray(spectrogram))) ** self.power
        if self.griffin_lim_device == "gpu":
            from ._lib import get_engine
            self._gl_check_params()
            F, M = S.shape
            if F != self.fft_size // 2 + 1:
                raise ValueError(f"inv_spectrogram: {F} frequency bins, expected {self.fft_size // 2 + 1}")
            u = torch.rand(1, M, F) if rng is None else torch.from_numpy(np.ascontiguousarray(
                np.asarray(rng.rand(F, M), np.float32).T)[None])
            Sd = torch.from_numpy(np.ascontiguousarray(S.T, dtype=np.float32)[None]).cuda()
            phase = u.float().cuda().contiguous()
            out = torch.empty(1, self.hop_length * (M - 1), device=Sd.device)
            eng = get_engine(Sd.device)
            with eng.lock:
                eng.griffin_lim(Sd, [M], self.fft_size, self.win_length, self.hop_length, self.griffin_lim_iters,
                                phase, out)
            wav = out[0].cpu().numpy()
        else:
            wav = self._griffin_lim(S, rng)
        if self.preemphasis != 0:
            import scipy.signal
            return scipy.signal.lfilter([1], [1, -self.preemphasis], wav)
        return wav

    # -- batched Griffin-Lim on the GPU (tts_mel_to_linear + tts_griffin_lim)
    def _denorm_affine(self, n_channels=None):
        """`_denormalize` on a mel as dB = clip(x) * scale + offset per channel: (scale, offset, clip)
        with clip None or the (lo, hi) bounds. With ``n_channels`` (a linear spectrogram's bins) the
        mean-var scaler is picked as `_scaler_for` picks it, its refusals included."""
        ones = np.ones(self.num_mels if n_channels is None else n_channels)
        if not self.signal_norm:
            return ones, 0.0 * ones, None
        if hasattr(self, "mel_scaler"):
            sc = self.mel_scaler if n_channels is None else self._scaler_for(np.empty((n_channels, 0)))
            return np.asarray(sc.scale_, np.float64), np.asarray(sc.mean_, np.float64), None
        if self.symmetric_norm:
            scale = -self.min_level_db / (2 * self.max_norm)
            offset = self.max_norm * scale + self.min_level_db + self.ref_level_db
            clip = (-self.max_norm, self.max_norm) if self.clip_norm else None
        else:
            scale = -self.min_level_db / self.max_norm
            offset = self.min_level_db + self.ref_level_db
            clip = (0.0, self.max_norm) if self.clip_norm else None
        return scale * ones, offset * ones, clip

    def _gl_check_params(self):
        """What the GPU Griffin-Lim covers (include/ttship.h, tts_griffin_lim)."""
        if self.stft_pad_mode != "reflect":
            raise NotImplementedError(f"GPU Griffin-Lim: stft_pad_mode={self.stft_pad_mode!r} (only 'reflect')")
        if self.fft_size != 1024:
            raise NotImplementedError(f"GPU Griffin-Lim: fft_size={self.fft_size} (only 1024)")
        if not 64 <= self.hop_length <= 512:
            raise NotImplementedError(f"GPU Griffin-Lim: hop_length={self.hop_length} (64 to 512)")

    def inv_melspectrogram_batch(self, mels, lengths, phase=None):
        """`inv_melspectrogram` of a batch on the GPU, without the pre-emphasis inverse: ``mels``
        (B, M_max, num_mels) normalised mels on a ROCm device, frame-major, row b valid for
        ``lengths[b]`` frames; ``phase`` (B, M_max, fft_size / 2 + 1) uniform [0, 1) numbers (drawn
        with torch.rand on the device when None). Returns the (B, hop_length * (M_max - 1)) device
        tensor (rows zero past their own length) and the per-row sample counts."""
        from ._lib import get_engine
        self._gl_check_params()
        eng = get_engine(mels.device)
        dev = mels.device
        if dev not in self._gl_dev_cache:
            scale, offset, clip = self._denorm_affine()
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
            self._gl_dev_cache[dev] = (put(self.inv_mel_basis), put(scale), put(offset), clip)
        inv_basis, scale, offset, clip = self._gl_dev_cache[dev]
        mels = mels.contiguous().float()
        B, M, _ = mels.shape
        lengths = [int(n) for n in lengths]
        F = self.fft_size // 2 + 1
        S = torch.empty(B, M, F, device=dev)
        if phase is None:
            phase = torch.rand(B, M, F, device=dev)
        phase = phase.contiguous().float()
        assert phase.shape == S.shape and phase.device == dev
        wav = torch.empty(B, self.hop_length * (M - 1), device=dev)
        with eng.lock:
            eng.mel_to_linear(mels, lengths, inv_basis, scale, offset, clip, self.spec_gain, self.power, S)
            eng.griffin_lim(S, lengths, self.fft_size, self.win_length, self.hop_length, self.griffin_lim_iters,
                            phase, wav)
        return wav, [self.hop_length * (n - 1) for n in lengths]

    def inv_spectrogram_batch(self, specs, lengths, phase=None, deemphasis=True):
        """`inv_spectrogram` of a batch on the GPU: ``specs`` (B, M_max, fft_size / 2 + 1) normalised
        linear spectrograms on a ROCm device, frame-major (a Tacotron (v1) postnet output), row b valid
        for ``lengths[b]`` frames; ``phase`` as in `inv_melspectrogram_batch`. The pre-emphasis
        inverse runs on the device too unless ``deemphasis`` is False or `preemphasis` is 0. Returns
        the (B, hop_length * (M_max - 1)) device tensor (rows zero past their own length) and the
        per-row sample counts."""
        from ._lib import get_engine
        self._gl_check_params()
        eng = get_engine(specs.device)
        dev = specs.device
        F = self.fft_size // 2 + 1
        if specs.dim() != 3 or specs.shape[-1] != F:
            raise ValueError(f"inv_spectrogram_batch: expected (B, M, {F}) spectrograms, got {tuple(specs.shape)}")
        if (dev, "linear") not in self._gl_dev_cache:
            scale, offset, clip = self._denorm_affine(F)
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
            self._gl_dev_cache[dev, "linear"] = (put(scale), put(offset), clip)
        scale, offset, clip = self._gl_dev_cache[dev, "linear"]
        specs = specs.contiguous().float()
        B, M, _ = specs.shape
        lengths = [int(n) for n in lengths]
        S = torch.empty(B, M, F, device=dev)
        if phase is None:
            phase = torch.rand(B, M, F, device=dev)
        phase = phase.contiguous().float()
        assert phase.shape == S.shape and phase.device == dev
        wav = torch.empty(B, self.hop_length * (M - 1), device=dev)
        counts = [self.hop_length * (n - 1) for n in lengths]
        with eng.lock:
            eng.spec_to_mag(specs, lengths, scale, offset, clip, self.spec_gain, self.power, S)
            eng.griffin_lim(S, lengths, self.fft_size, self.win_length, self.hop_length, self.griffin_lim_iters,
                            phase, wav)
            if deemphasis and self.preemphasis != 0:
                eng.deemphasis(wav, counts, self.preemphasis, wav)
        return wav, counts

    # -- the waveform tail on the GPU (tts_deemphasis, tts_wav_finish)
    def deemphasis_batch(self, wav, counts):
        """The pre-emphasis inverse, ``scipy.signal.lfilter([1], [1, -preemphasis], row)``, on every
        row of the (B, L_max) device tensor ``wav``, row b for ``counts[b]`` samples (fp32). Returns
        a new tensor, zero past each row's count; with `preemphasis` 0 the filter is the identity."""
        from ._lib import get_engine
        eng = get_engine(wav.device)
        wav = wav.contiguous().float()
        counts = [int(n) for n in counts]
        assert wav.dim() == 2 and len(counts) == wav.shape[0]
        if self.preemphasis == 0:
            return wav.clone()
        out = torch.empty_like(wav)
        with eng.lock:
            eng.deemphasis(wav, counts, self.preemphasis, out)
        return out

    def finish_batch(self, wav, counts, gap=10000, threshold_db=-40, min_silence_sec=0.8):
        """The end of `Synthesizer.tts` on the GPU: every row of the (B, L_max) device tensor ``wav``
        (row b valid for ``counts[b]`` samples) is cut at its `find_endpoint`, the rows are joined in
        order with ``gap`` zeros after each, and the result is scaled and truncated as `save_wav`
        does. Returns the int16 numpy array `save_wav` would write and the list of endpoints."""
        from ._lib import get_engine
        eng = get_engine(wav.device)
        wav = wav.contiguous().float()
        counts = [int(n) for n in counts]
        assert wav.dim() == 2 and len(counts) == wav.shape[0]
        window_length = int(self.sample_rate * min_silence_sec)
        hop_length = int(window_length / 4)
        B = wav.shape[0]
        pcm = torch.empty(max(1, sum(counts) + B * int(gap)), dtype=torch.int16, device=wav.device)
        meta = torch.empty(B + 1, dtype=torch.int32, device=wav.device)  # the endpoints, then the total
        with eng.lock:
            eng.wav_finish(wav, counts, window_length, hop_length, float(self._db_to_amp(threshold_db)), gap, pcm,
                           meta[:B], meta[B:])
        meta = meta.cpu().tolist()
        return pcm[:meta[B]].cpu().numpy(), meta[:B]

    # -- trimming / saving (audio.py:302-341)
    def find_endpoint(self, wav, threshold_db=-40, min_silence_sec=0.8):
        """audio.py:302-309: first window of min_silence_sec whose peak is below threshold_db."""
        window_length = int(self.sample_rate * min_silence_sec)
        hop_length = int(window_length / 4)
        threshold = self._db_to_amp(threshold_db)
        for x in range(hop_length, len(wav) - window_length, hop_length):
            if np.max(wav[x:x + window_length]) < threshold:
                return x + hop_length
        return len(wav)

    def trim_silence(self, wav):
        margin = int(self.sample_rate * 0.01)
        wav = wav[margin:-margin]
        n, hop, fl = len(wav), self.hop_length, self.win_length
        if n == 0:
            return wav
        yp = np.pad(wav, fl // 2, mode="reflect") if n > fl // 2 else np.pad(wav, fl // 2)
        nfr = 1 + (len(yp) - fl) // hop
        if nfr < 1:
            return wav
        idx = np.arange(fl)[None, :] + hop * np.arange(nfr)[:, None]
        mse = np.mean(np.abs(yp[idx]) ** 2, axis=1)
        db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
        nz = np.flatnonzero(db > -self.trim_db)
        if nz.size == 0:
            return wav[:0]
        return wav[nz[0] * hop:min(n, (nz[-1] + 1) * hop)]

    def save_wav(self, wav, path):
        wav_norm = np.asarray(wav) * (32767 / max(0.01, np.max(np.abs(wav))))
        scipy.io.wavfile.write(path, self.sample_rate, wav_norm.astype(np.int16))


def wav_bytes(ap, wav):
    out = io.BytesIO()
    ap.save_wav(wav, out)
    return out
