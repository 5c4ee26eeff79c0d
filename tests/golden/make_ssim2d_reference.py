"""Writes tests/golden/ssim2d_reference.npz: the values of the reference's own ssim() (models/pytorch_msssim/__init__.py:29-80) on
the plane pairs of tests/metrics_yuv_common.golden_pairs(), evaluated on the CPU in float64 with the reference's window
create_window(11, 1).double() at val_range = 1, beside the pairs themselves.

    python tests/golden/make_ssim2d_reference.py PATH_OF_A_DRBA_CHECKOUT

Needs a checkout of the reference (routineLife1/DRBA) and no GPU; the tests read only the .npz.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import metrics_yuv_common as myc  # noqa: E402


def main(reference_root):
    spec = importlib.util.spec_from_file_location("ref_msssim", os.path.join(reference_root, "models", "pytorch_msssim", "__init__.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    window = ref.create_window(11, 1).cpu().double()
    out = {}
    for key, p, q, maxval in myc.golden_pairs():
        x, y = myc.as_unit(p, maxval).double(), myc.as_unit(q, maxval).double()
        out[key + "/p"], out[key + "/q"], out[key + "/maxval"] = p, q, np.int64(maxval)
        out[key + "/ssim"] = np.float64(float(ref.ssim(x, y, window=window, val_range=1)))
        print(f"{key:24s} ssim = {float(out[key + '/ssim']):.12f}  dense restatement differs by "
              f"{abs(float(out[key + '/ssim']) - myc.ssim2d_truth(p, q, maxval)):.1e}")
    np.savez_compressed(myc.GOLDEN, **out)


if __name__ == "__main__":
    main(sys.argv[1])
