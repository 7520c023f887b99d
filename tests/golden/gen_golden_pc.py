#!/usr/bin/env python3
"""Generate tests/golden/quant_pc.npz by running the REFERENCE's own quantize_tensor / quantize_tensor_b with
channel_level=True (retune_bias_quantize.py:73-97), imported the way gen_golden.py imports it, on the synthetic tensors of
tests/int8_pc_ref.py (QUANT_PC_CASES).  Stored per case: q (int32) and log2(scale) (int32, in the shape the reference
returns the scale in).  Recorded data only: nothing of the reference's source travels.

    python tests/golden/gen_golden_pc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import import_reference  # noqa: E402

import torch  # noqa: E402
import int8_pc_ref as P  # noqa: E402


def main():
    rbq = import_reference().rbq
    out = {}
    for tag, seed, shape, gain in P.QUANT_PC_CASES:
        t = torch.from_numpy(P.quant_pc_input(seed, shape, gain))
        # the reference's per-channel bias form multiplies a 1-D scale into the tensor: it only takes 1-D tensors
        fn = rbq.quantize_tensor_b if t.dim() == 1 else rbq.quantize_tensor
        q, scale = fn(t, 8, True)
        e = torch.log2(scale)
        assert torch.equal(e, torch.round(e)) and float(q.abs().max()) <= 127
        out[tag + "/q"] = q.numpy().astype(np.int32)
        out[tag + "/e"] = e.numpy().astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "quant_pc.npz"), **out)
    print("quant_pc.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
