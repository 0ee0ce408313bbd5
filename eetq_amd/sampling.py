"""The 32-byte parameter block of ``ops.sample_handover`` (eetq_sample_handover_f16), in plain Python for both bindings.

Layout (little endian, include/eetq_amd.h): float32 temperature, float32 top_p, int32 top_k, int32 eos_token, int32 pad_token,
int32 reserved (0), uint64 seed -- held in an int32[8] device tensor the kernel reads, so a captured HIP graph serves any
setting: rewrite the block (``out=``), replay.
"""
import struct

import torch

__all__ = ["sampling_params", "pack_sampling_params"]

_FORMAT = "<ffiiiiQ"


def pack_sampling_params(temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_token_id=None, pad_token_id=0):
    """The block's 32 bytes."""
    return struct.pack(_FORMAT, float(temperature), float(top_p), int(top_k), -1 if eos_token_id is None else int(eos_token_id),
                       int(pad_token_id), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)


def sampling_params(temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_token_id=None, pad_token_id=0, device=None, out=None):
    """Fill (``out=``: an existing int32[8] block, rewritten in place) or return the parameter block on ``device`` in one
    host-to-device copy.  ``temperature`` 0 selects greedy, ``top_k`` <= 0 and ``top_p`` >= 1 switch the filters off,
    ``eos_token_id`` None means no EOS token, ``seed`` is the 64-bit Philox key."""
    host = torch.frombuffer(bytearray(pack_sampling_params(temperature, top_k, top_p, seed, eos_token_id, pad_token_id)),
                            dtype=torch.int32)
    if out is not None:
        if out.dtype != torch.int32 or out.numel() != 8 or not out.is_contiguous():
            raise ValueError("sampling_params: out must be a contiguous int32[8] tensor")
        out.view(-1).copy_(host)
        return out
    return host.to(device if device is not None else "cuda")
