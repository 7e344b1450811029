"""Audio augmentation: the mirror of the reference's augmentation layer (ultravox/data/aug/: base.py, config.py, registry.py, gain.py, noise.py,
filter.py) with the arithmetic on the GPU.  `UltravoxDataproc(..., augmentation=...)` calls `augmentation.apply_sample(sample)` on every training
sample; `AugRegistry.create_parent_augmentation([...])` builds what goes there.

What is the reference's: the surface (AugmentationArgs, AugmentationConfig, AugRegistry, Augmentation with __call__ / apply_sample / apply /
_apply and the "null" shell), the type names with their parameter names and defaults, the named configs (tests/golden/aug_configs.json), the order
in which a chain runs (children first, each through its own __call__, then the parent's _apply; `None` passes through) and the HOST randomness in
its call order: one `random.random()` per __call__ (skip when it exceeds p), one `np.random.uniform(lo, hi)` inside _apply of `random_gain` and
`random_colored_noise`.  A host seeded like the reference makes the same apply / skip decisions and draws the same gain_db / snr_db.

What is this package's: where the arithmetic runs.  Always on the GPU (uvx_aug_gain, uvx_aug_iir, uvx_aug_noise of include/uvx.h, where the three
definitions are written down); there is no CPU form.  Every type takes `device=` (default "cuda") and the noise types `seed=`, as constructor
arguments or as params of a config.  A numpy clip (int16, float32, or float64 cast to float32) goes up as it is; a CUDA f32 tensor stays where it
is; `_apply` returns a 1-D f32 CUDA tensor, and between the stages of a chain the clip stays on the device in f32.  (The reference carries float64
between stages after a filter or a noise stage; that is a difference in the last bits of what the next stage reads.)  A stage that is skipped
returns its input object unchanged, so a chain in which nothing applies leaves a numpy clip a numpy clip.

The gain is the reference's to the bit.  The filter is scipy.signal.lfilter with scipy's own Butterworth design, parallel in time by warm-up
blocks (`iir_warm_len`).  The noise has the reference's law on a power-of-two frequency grid and its own random stream (Philox under `seed`, one
`offset` per launch), so no two launches of one augmentation repeat their noise and a given (seed, launch count) gives the same bits again.

`apply_batch(clips)` runs each stage as ONE launch over the ragged batch: the per-clip decisions of a stage are drawn in clip order and select
the rows its launch covers (stage by stage, where `__call__` on each clip in turn would go clip by clip).

`resampling` (librosa's soxr_hq, which is not scipy's polyphase filter and cannot be restated here) and `compression` (ffmpeg / audioop codecs) are
registered type names whose construction raises NotImplementedError: an unbuilt augmentation is refused, not skipped."""
from __future__ import annotations

import copy
import dataclasses
import os
import random
from typing import Any, Dict, List, Optional, Type, Union

import numpy as np

SAMPLE_RATE = 16000
NOISE_TYPES = ("white", "pink", "brown", "blue", "violet")
IIR_WARM_SPAN = 1 << 17        # samples of the impulse response iir_warm_len looks at
IIR_WARM_LIMIT = 1 << 16       # the warm-up has to be shorter than this
IIR_WARM_TAIL = 2.0 ** -40     # share of sum |h| that may lie beyond the warm-up


# ------------------------------------------------------------------------------------------------ configs
@dataclasses.dataclass
class AugmentationArgs:
    p: float = 1.0
    sample_rate: int = SAMPLE_RATE

    def to_dict(self) -> Dict[str, Any]:
        return {"p": self.p, "sample_rate": self.sample_rate}

    def param_names(self) -> List[str]:
        return [f.name for f in dataclasses.fields(self)]


@dataclasses.dataclass
class AugmentationConfig:
    name: str
    type: Optional[str] = None
    params: Dict[str, Any] = dataclasses.field(default_factory=dict)
    description: Optional[str] = None
    args: AugmentationArgs = dataclasses.field(default_factory=AugmentationArgs)
    children: Optional[List["AugmentationConfig"]] = None

    def update_params(self, data: Dict[str, Any]) -> None:
        self.params.update(data)

    def update(self, data: Dict[str, Any]) -> "AugmentationConfig":
        """Keys of AugmentationArgs go to `args`, `description` and `children` to their fields, everything else to `params`; `data` is consumed."""
        assert "type" not in data, "type cannot be updated"
        assert "name" not in data, "name cannot be updated"
        for key in self.args.param_names():
            if key in data:
                setattr(self.args, key, data.pop(key))
        if "description" in data:
            self.description = data.pop("description")
        if "children" in data:
            assert all(isinstance(c, AugmentationConfig) for c in data["children"]), "Must update children with AugmentationConfig objects"
            self.children = data.pop("children")
        self.update_params(data)
        return self


# ------------------------------------------------------------------------------------------------ base
class Augmentation:
    """The shell type ("null"): runs its children and changes nothing itself."""

    def __init__(self, args: AugmentationArgs, children: Optional[List["Augmentation"]] = None, device="cuda"):
        assert 0 <= args.p <= 1, "Probability must be between 0 and 1"
        self.p = args.p
        self.children = children or []
        self.sample_rate = args.sample_rate
        self.device = device

    def __call__(self, audio):
        if random.random() > self.p:
            return audio
        return self.apply(audio)

    def apply_sample(self, sample):
        if sample.audio is None:
            return sample
        sample.audio = self(sample.audio)
        return sample

    def apply(self, audio):
        if audio is None:
            return None
        for child in self.children:
            audio = child(audio)
            if audio is None:
                return None
        return self._apply(audio)

    def _apply(self, audio):
        return self._apply_rows([audio])[0]

    # -- the batch form: one launch per stage
    def apply_batch(self, clips) -> list:
        """`self(clip)` for every clip of a list, each stage as one launch over the clips it applies to.  -> the list of results"""
        clips = list(clips)
        self._batch(clips, [i for i in range(len(clips)) if random.random() <= self.p])
        return clips

    def _batch(self, clips: list, idx: List[int]) -> None:
        idx = [i for i in idx if clips[i] is not None]
        for child in self.children:
            child._batch(clips, [i for i in idx if random.random() <= child.p])
        if idx:
            for i, y in zip(idx, self._apply_rows([clips[i] for i in idx])):
                clips[i] = y

    def _apply_rows(self, rows: list) -> list:
        """The augmentation itself on a list of clips, one launch; the host draws of the rows are made here, in row order."""
        return rows


class _DeviceAugmentation(Augmentation):
    """A type whose arithmetic is one libuvx entry: `_draw()` makes the host draw of one row, `_launch(pcm, row_offset, n, values, max_n)` runs
    the rows."""

    def __init__(self, args: AugmentationArgs, device="cuda"):
        super().__init__(args, device=device)
        import torch

        if torch.device(device).type != "cuda":
            raise ValueError(f"{type(self).__name__}: device={device!r}, but the augmentations run on the GPU only: there is no CPU form")

    def _draw(self):
        raise NotImplementedError

    def _launch(self, pcm, row_offset, n, values, max_n):
        raise NotImplementedError

    def _apply_rows(self, rows: list) -> list:
        values = [self._draw() for _ in rows]
        return self._run(rows, values)

    def _run(self, rows: list, values: list) -> list:
        import torch
        from .frontend import _pack_clips

        on_device = [x.device for x in rows if isinstance(x, torch.Tensor) and x.is_cuda]
        pcm, row_offset, n, lens = _pack_clips(rows, on_device[0] if on_device else self.device, type(self).__name__)
        out = self._launch(pcm, row_offset, n, values, max(lens))
        return [out[i, :k] for i, k in enumerate(lens)]


# ------------------------------------------------------------------------------------------------ registry
class AugRegistry:
    """Augmentation types by name, and named configs of them (several configs may share a type)."""

    _aug_types: Dict[str, Type[Augmentation]] = {}
    _configs: Dict[str, AugmentationConfig] = {}

    @classmethod
    def register_type(cls, name: str):
        def wrapper(aug_cls):
            cls.register_type_manual(name, aug_cls)
            return aug_cls
        return wrapper

    @classmethod
    def register_type_manual(cls, name: str, aug_cls) -> None:
        cls._aug_types[name] = aug_cls

    @classmethod
    def register_config(cls, name: str, config: AugmentationConfig) -> None:
        cls._configs[name] = config

    @classmethod
    def get_type(cls, name: Union[str, None]):
        name = "null" if name is None else name
        if name not in cls._aug_types:
            raise KeyError(f"Augmentation type '{name}' not found in registry")
        return cls._aug_types[name]

    @classmethod
    def get_config(cls, name: str, override_args: Optional[Dict[str, Any]] = None) -> AugmentationConfig:
        """The named config, or - for an unknown name - a new one made from override_args, which then has to hold exactly one of `type` and
        `children`.  With override_args the result is an updated copy; the registered config is never changed.  Children given as dicts are
        resolved through get_config by their own `name`."""
        if name in cls._configs:
            config = cls._configs[name]
        else:
            assert override_args, f"No override args specified for augmentation {name}"
            assert ("type" in override_args) ^ ("children" in override_args), \
                f"Only one of `type` or `children` must be in override args for augmentation {name}"
            config = AugmentationConfig(name=name, type=override_args.pop("type")) if "type" in override_args else AugmentationConfig(name=name)
        if not override_args:
            return config
        config = copy.deepcopy(config)
        if "children" in override_args:
            override_args["children"] = [c if isinstance(c, AugmentationConfig) else cls.get_config(c.pop("name"), c)
                                         for c in override_args["children"]]
        return config.update(override_args)

    @classmethod
    def create_augmentation(cls, config: AugmentationConfig) -> Augmentation:
        assert not (config.children and config.type), f"Cannot specify both children {config.children} and type {config.type}"
        if config.children:
            return cls.get_type(config.type)(args=config.args, children=[cls.create_augmentation(c) for c in config.children])
        return cls.get_type(config.type)(args=config.args, **config.params)

    @classmethod
    def create_parent_augmentation(cls, augmentations: List[Augmentation]) -> Augmentation:
        return cls.get_type("null")(args=AugmentationArgs(), children=augmentations)


AugRegistry.register_type_manual("null", Augmentation)
AugRegistry.register_config("null", AugmentationConfig(name="null", type=None, params={}, description="Shell augmentation"))


# ------------------------------------------------------------------------------------------------ gain
def gain_linear(gain_db: float) -> np.float32:
    """10^(gain_db / 20) in float64, rounded once to f32: what numpy multiplies a float32 clip by."""
    return np.float32(10 ** (gain_db / 20))


class _GainBase(_DeviceAugmentation):
    def _launch(self, pcm, row_offset, n, values, max_n):
        from . import ops
        return ops.aug_gain(pcm, row_offset, n, np.array([gain_linear(g) for g in values], dtype=np.float32), max_n=max_n)


@AugRegistry.register_type("gain")
class Gain(_GainBase):
    def __init__(self, args: AugmentationArgs, gain_db: float = 0.0, device="cuda"):
        super().__init__(args, device=device)
        self.gain_db = gain_db

    def _draw(self):
        return self.gain_db


@AugRegistry.register_type("random_gain")
class RandomGain(_GainBase):
    def __init__(self, args: AugmentationArgs, min_gain_db: float = -24.0, max_gain_db: float = 15.0, device="cuda"):
        super().__init__(args, device=device)
        assert min_gain_db <= max_gain_db
        self.min_gain_db, self.max_gain_db = min_gain_db, max_gain_db

    def _draw(self):
        return np.random.uniform(self.min_gain_db, self.max_gain_db)


AugRegistry.register_config("gain", AugmentationConfig(name="gain", type="gain", params={"gain_db": 0.0}, description="Apply no gain."))
AugRegistry.register_config("gain_10db", AugmentationConfig(name="gain_10db", type="gain", params={"gain_db": 10.0}, description="Apply 10dB gain."))
AugRegistry.register_config("gain_minus_10db",
                            AugmentationConfig(name="gain_minus_10db", type="gain", params={"gain_db": -10.0}, description="Apply -10dB gain."))
AugRegistry.register_config("random_gain", AugmentationConfig(name="random_gain", type="random_gain",
                                                              params={"min_gain_db": -24.0, "max_gain_db": 15.0}, description="Apply random gain."))


# ------------------------------------------------------------------------------------------------ noise
class _NoiseBase(_DeviceAugmentation):
    def __init__(self, args: AugmentationArgs, noise_type: str, seed: Optional[int], device):
        super().__init__(args, device=device)
        assert noise_type in NOISE_TYPES
        self.noise_type = noise_type
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)      # (not from the host generators: their order is the reference's)
        self.offset = 0                                                                          # one per launch

    def _launch(self, pcm, row_offset, n, values, max_n):
        from . import ops
        offset, self.offset = self.offset, self.offset + 1
        ratio = np.array([10 ** (-snr_db / 10) for snr_db in values], dtype=np.float64)
        return ops.aug_noise(pcm, row_offset, n, ratio, colour=self.noise_type, seed=self.seed, offset=offset, max_n=max_n)


@AugRegistry.register_type("colored_noise")
class ColoredNoise(_NoiseBase):
    def __init__(self, args: AugmentationArgs, noise_type: str = "white", snr_db: float = 20, seed: Optional[int] = None, device="cuda"):
        super().__init__(args, noise_type, seed, device)
        self.snr_db = snr_db

    def _draw(self):
        return self.snr_db


@AugRegistry.register_type("random_colored_noise")
class RandomColoredNoise(_NoiseBase):
    def __init__(self, args: AugmentationArgs, noise_type: str = "white", min_snr_db: float = 0.0, max_snr_db: float = 20.0,
                 seed: Optional[int] = None, device="cuda"):
        super().__init__(args, noise_type, seed, device)
        self.min_snr_db, self.max_snr_db = min_snr_db, max_snr_db

    def _draw(self):
        return np.random.uniform(self.min_snr_db, self.max_snr_db)


AugRegistry.register_config("white_noise", AugmentationConfig(name="white_noise", type="colored_noise", params={"noise_type": "white", "snr_db": 20}))
AugRegistry.register_config("pink_noise", AugmentationConfig(name="pink_noise", type="colored_noise", params={"noise_type": "pink", "snr_db": 20}))
AugRegistry.register_config("random_pink_noise",
                            AugmentationConfig(name="random_pink_noise", type="random_colored_noise",
                                               params={"noise_type": "pink", "min_snr_db": 0.0, "max_snr_db": 20.0}))


# ------------------------------------------------------------------------------------------------ filters
def iir_warm_len(b, a) -> int:
    """The look-back of uvx_aug_iir for the filter (b, a): the smallest W such that the sum of |h[k]| over k >= W is at most 2^-40 of the sum
    over all k, h the float64 impulse response over 2^17 samples.  A block of the kernel that starts W samples early has dropped at most that
    share of the response.  ValueError if there is no such W below 2^16: such a filter is refused, there is no other kernel behind this one."""
    from scipy.signal import lfilter

    x = np.zeros(IIR_WARM_SPAN)
    x[0] = 1.0
    h = np.abs(lfilter(np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64), x))
    if not np.all(np.isfinite(h)) or h.sum() == 0.0:
        raise ValueError("iir_warm_len: the impulse response is not finite or is zero; the filter is not a stable one")
    tail = np.concatenate([np.cumsum(h[::-1])[::-1], [0.0]])       # tail[W] = sum over k >= W
    ok = np.nonzero(tail <= IIR_WARM_TAIL * tail[0])[0]
    if len(ok) == 0 or ok[0] >= IIR_WARM_LIMIT:
        raise ValueError(f"iir_warm_len: the impulse response has more than 2^-40 of its absolute sum beyond {IIR_WARM_LIMIT} samples (the limit of "
                         f"the warm-up of uvx_aug_iir); a filter that rings this long is not built")
    return int(ok[0])


class _FilterBase(_DeviceAugmentation):
    def _design(self, b, a) -> None:
        from . import ops
        b, a = np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64)
        self.b, self.a = b / a[0], a / a[0]
        if not 1 <= len(self.a) - 1 <= ops.AUG_IIR_MAX_ORDER or len(self.b) != len(self.a):
            raise ValueError(f"{type(self).__name__}: the filter has {len(self.b)} / {len(self.a)} coefficients; uvx_aug_iir is built for equal "
                             f"counts and orders 1 to {ops.AUG_IIR_MAX_ORDER} (a band-pass has twice the order it is designed with)")
        self.warm = iir_warm_len(self.b, self.a)
        self._on_device = {}

    def _draw(self):
        return None

    def _launch(self, pcm, row_offset, n, values, max_n):
        import torch
        from . import ops
        if pcm.device not in self._on_device:
            self._on_device[pcm.device] = (torch.from_numpy(self.b).to(pcm.device), torch.from_numpy(self.a).to(pcm.device))
        b, a = self._on_device[pcm.device]
        return ops.aug_iir(pcm, row_offset, n, b, a, self.warm, max_n=max_n)


@AugRegistry.register_type("bandpass_filter")
class BandpassFilter(_FilterBase):
    def __init__(self, args: AugmentationArgs, lowcut: float = 300, highcut: float = 3400, order: int = 5, device="cuda"):
        super().__init__(args, device=device)
        from scipy.signal import butter
        self.lowcut, self.highcut, self.order = lowcut, highcut, order
        nyquist = self.sample_rate / 2
        self._design(*butter(order, [lowcut / nyquist, highcut / nyquist], btype="band"))


@AugRegistry.register_type("lowpass_filter")
class LowpassFilter(_FilterBase):
    def __init__(self, args: AugmentationArgs, cutoff: float = 3400, order: int = 2, device="cuda"):
        super().__init__(args, device=device)
        from scipy.signal import butter
        self.cutoff, self.order = cutoff, order
        self._design(*butter(order, cutoff / (self.sample_rate / 2), btype="low"))


AugRegistry.register_config("telephone_bandpass", AugmentationConfig(name="telephone_bandpass", type="bandpass_filter",
                                                                     params={"lowcut": 300, "highcut": 3400, "order": 5}))
AugRegistry.register_config("telephone_lowpass", AugmentationConfig(name="telephone_lowpass", type="lowpass_filter", params={"cutoff": 3400, "order": 2}))


# ------------------------------------------------------------------------------------------------ what is not built
def _unbuilt(type_name: str, why: str):
    class Unbuilt(Augmentation):
        def __init__(self, args: AugmentationArgs = None, **params):
            raise NotImplementedError(f"the '{type_name}' augmentation is not built: {why}")
    Unbuilt.__name__ = Unbuilt.__qualname__ = f"Unbuilt_{type_name}"
    return Unbuilt


AugRegistry.register_type_manual("resampling", _unbuilt(
    "resampling", "the reference resamples with librosa's soxr_hq, which is not scipy's polyphase filter (uvx_resample_poly) and cannot be restated here"))
for _name in ("compression", "ffmpeg_compression", "audioop_compression", "amr_compression"):
    AugRegistry.register_type_manual(_name, _unbuilt(_name, "the reference runs ffmpeg / audioop codecs on the host, and there is no device form of them"))
