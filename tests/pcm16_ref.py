"""The conversion rule of 16-bit PCM frames (include/flowz_hip.h: fz_run_block_pcm16), stated once in numpy for the tests.

in    x = (float32)q * 2^-15: exact, -32768 gives -1.0f
out   r = y * 32768.0f (one float32 multiplication); NaN -> 0; r >= 32767 -> 32767; r <= -32768 -> -32768; else r rounded to the nearest
      integer, ties to even.  No dither."""
import numpy as np

F32 = np.float32


def to_float(q):
    q = np.asarray(q)
    assert q.dtype == np.int16
    return q.astype(F32) * F32(2.0 ** -15)


def from_float(y):
    y = np.asarray(y)
    assert y.dtype == F32
    with np.errstate(all="ignore"):
        return np.where(np.isnan(y), 0, np.clip(np.rint(y * F32(32768)), -32768, 32767)).astype(np.int16)
