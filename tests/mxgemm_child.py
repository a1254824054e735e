"""Child process of tests/test_gpu_mxfp8_persistent.py: DIT_SMALL's "full" case with the three fp8 modes on, under
whatever SA_MXGEMM_KERNEL the parent set (the library reads it once per process); the output goes to argv[1]."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def main(path):
    from golden_cases import DIT_SMALL, dit_inputs
    from test_gpu_dit import make_model, run
    m = make_model(DIT_SMALL)
    m.enable_fp8_qkv(), m.enable_fp8_attention(), m.enable_fp8_ffn()
    torch.save(run(m, dit_inputs(DIT_SMALL, "full")), path)


if __name__ == "__main__":
    main(sys.argv[1])
