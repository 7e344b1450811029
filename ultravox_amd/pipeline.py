"""UltravoxPipeline: the reference's front door (ultravox_pipeline.py), the class its model cards tell users to call:

    pipe({"audio": pcm, "turns": turns, "sampling_rate": sr}, max_new_tokens=30)

A restatement in this package's own words: no `transformers.Pipeline` base and no registry call - `__call__` runs the four stages the base
class would run (`_sanitize_parameters` -> `preprocess` -> `_forward` -> `postprocess`) on one input and returns the reply as a string.

The pipeline calls `generate()` in exactly two ways (ultravox_pipeline.py:97-121), and both select their tokens in one launch per token:
  no temperature   do_sample=False, repetition_penalty=1.1          uvx_seen_mark + uvx_greedy_select_penalized
  a temperature    do_sample=True, temperature=t, repetition_penalty=1.1
                   with `sampler_seed` given: a PhiloxGenerator(seed, penalty_on_device=True) owned by the pipeline is passed as `generator=`,
                   so the call runs uvx_seen_mark + uvx_sample_select_penalized; with sampler_seed=None it keeps torch's sampler, token for
                   token what generate() does without a generator.

Deviation: `max_new_tokens=None` leaves the keyword out, so generate()'s own default of 20 NEW tokens applies.  The reference hands None on to
[3P] HF `generate`, which falls back to its generation config's max_length = 20 - prompt included, i.e. usually nothing new at all and a warning.
A terminator is listed once where eos and <|eot_id|> are the same id (the reference lists it twice; the tokens are the same).
"""
import logging
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .processing import AUDIO_PLACEHOLDER, UltravoxProcessor

GENERATION_KEYS = frozenset(("temperature", "max_new_tokens", "repetition_penalty"))
DEFAULT_SAMPLING_RATE = 16000
DEFAULT_REPETITION_PENALTY = 1.1
EOT = "<|eot_id|>"
# integer PCM -> [-1, 1): one f32 division by the type's full scale
PCM_FULL_SCALE = {np.dtype(np.int16): np.float32(2.0 ** 15), np.dtype(np.int32): np.float32(2.0 ** 31)}
# the reference's two warnings, word for word: callers and tests see them
NO_PLACEHOLDER = "Prompt does not contain '<|audio|>', appending '<|audio|>' to the end of the prompt."
NO_SAMPLING_RATE = "No sampling rate provided, using default of 16kHz. We highly recommend providing the correct sampling rate."


def pcm_to_float32(audio):
    """A numpy waveform as f32: integer PCM scaled by its full scale, float64 narrowed; f32 arrays and anything that is not a numpy array pass."""
    if not isinstance(audio, np.ndarray):
        return audio
    full_scale = PCM_FULL_SCALE.get(audio.dtype)
    if full_scale is not None:
        return audio.astype(np.float32) / full_scale
    return audio.astype(np.float32) if audio.dtype == np.float64 else audio


def conversation(inputs: Dict[str, Any], has_audio: bool) -> List[Dict[str, str]]:
    """The turns the chat template gets.  Audio needs a user turn at the end to stand in: where the caller's turns do not end with one, a user turn
    made of `prompt` (default: the bare placeholder) is appended - to the caller's own list, which therefore holds it afterwards - and a prompt
    without the placeholder gets it at its end, with a warning.  Without audio the turns are taken as they are and `prompt` is not read."""
    turns = inputs["turns"] if "turns" in inputs else []
    ends_with_user = bool(turns) and turns[-1]["role"] == "user"
    if has_audio and not ends_with_user:
        content = inputs.get("prompt", AUDIO_PLACEHOLDER)
        if AUDIO_PLACEHOLDER not in content:
            logging.warning(NO_PLACEHOLDER)
            content = f"{content} {AUDIO_PLACEHOLDER}"
        turns.append(dict(role="user", content=content))
    return turns


class UltravoxPipeline:
    def __init__(self, model, tokenizer, processor: Optional[UltravoxProcessor] = None, audio_processor=None, chat_template: Optional[str] = None,
                 sampler_seed: Optional[int] = None):
        if chat_template:
            tokenizer.chat_template = chat_template
        self.model, self.tokenizer = model, tokenizer
        if processor is None:
            processor = UltravoxProcessor(audio_processor=audio_processor, tokenizer=tokenizer, stack_factor=model.config.stack_factor,
                                          audio_context_size=model.audio_tower_context_length)
        self.processor = processor
        # sampler_seed: sampled calls draw on the device from one Philox stream owned by this instance; None: torch's sampler
        self.sampler = None
        if sampler_seed is not None:
            from .generation import PhiloxGenerator
            self.sampler = PhiloxGenerator(sampler_seed, penalty_on_device=True)

    def __call__(self, inputs: Dict[str, Any], **kwargs) -> str:
        _, forward_kwargs, _ = self._sanitize_parameters(**kwargs)
        model_inputs = self.preprocess(inputs)
        device = self.model.device      # ([3P] Pipeline.forward moves every tensor of the model inputs to the model's device)
        model_inputs = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in model_inputs.items()}
        return self.postprocess(self._forward(model_inputs, **forward_kwargs))

    def _sanitize_parameters(self, **kwargs):
        """-> (preprocess, forward, postprocess) keywords: only the three generation keys reach _forward, everything else is dropped."""
        forward = {name: value for name, value in kwargs.items() if name in GENERATION_KEYS}
        return {}, forward, {}

    def preprocess(self, inputs: Dict[str, Any]):
        """{"audio", "turns", "prompt", "sampling_rate"} -> the processor's output, audio_values in the model's dtype on its device."""
        audio = pcm_to_float32(inputs.get("audio"))
        has_audio = audio is not None
        chat = self.processor.tokenizer.apply_chat_template(conversation(inputs, has_audio), tokenize=False, add_generation_prompt=True)
        rate_given = "sampling_rate" in inputs
        if has_audio and not rate_given:
            logging.warning(NO_SAMPLING_RATE)
        rate = inputs["sampling_rate"] if rate_given else DEFAULT_SAMPLING_RATE
        features = self.processor(text=chat, audio=audio, sampling_rate=rate)
        if "audio_values" in features:
            features["audio_values"] = features["audio_values"].to(device=self.model.device, dtype=self.model.dtype)
        return features

    def _terminators(self) -> List[int]:
        """The tokenizer's eos and, where it has one, <|eot_id|> (LocalInference._terminators: an id is listed once)."""
        ids = [self.tokenizer.eos_token_id]
        if EOT in getattr(self.tokenizer, "added_tokens_encoder", {}):
            eot = self.tokenizer.convert_tokens_to_ids(EOT)
            if eot not in ids:
                ids.append(eot)
        return ids

    def _generation_kwargs(self, temperature, max_new_tokens, repetition_penalty) -> Dict[str, Any]:
        """The two calls the pipeline makes: greedy under the penalty (no temperature, or 0), or sampling at the temperature under the penalty - with
        the pipeline's own generator where it has one.  generate()'s temperature is a float, so a greedy call leaves it out, as it leaves out a
        max_new_tokens of None."""
        sampled = bool(temperature)
        kw: Dict[str, Any] = dict(do_sample=sampled, repetition_penalty=repetition_penalty, eos_token_id=self._terminators())
        if sampled:
            kw["temperature"] = temperature
            if self.sampler is not None:
                kw["generator"] = self.sampler
        if max_new_tokens is not None:
            kw["max_new_tokens"] = max_new_tokens
        return kw

    def _forward(self, model_inputs: Dict[str, Any], temperature: Optional[float] = None, max_new_tokens: Optional[int] = None,
                 repetition_penalty: float = DEFAULT_REPETITION_PENALTY):
        """-> the new tokens of row 0."""
        sequences = self.model.generate(**model_inputs, **self._generation_kwargs(temperature, max_new_tokens, repetition_penalty))
        prompt_len = model_inputs["input_ids"].shape[-1]
        return sequences[0][prompt_len:]

    def postprocess(self, model_outputs) -> str:
        return self.tokenizer.decode(model_outputs, skip_special_tokens=True)
