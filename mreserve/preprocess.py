"""`mreserve.preprocess` of the reference (mreserve/preprocess.py) under its own import name: the integer / layout side
(merlot_reserve_amd.preprocess); `encoder` is resolved lazily (the tokenizer vocabulary is the user's file)."""
from merlot_reserve_amd import preprocess as _p
from merlot_reserve_amd.preprocess import (END, LTOVPOOL, MASK, MASKAUDIO, PADDING, RESETCTX, START, make_spectrogram,   # noqa: F401
                                           make_spectrograms, patchify, preprocess_image_to_patches, preprocess_video,
                                           segments_from_decoded, segments_from_decoded_zero_shot, segments_from_pcm,
                                           video_to_segments)


def __getattr__(name):
    return getattr(_p, name)
