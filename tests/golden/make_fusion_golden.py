"""Golden vectors for the soft (if_pre_sampling 2) and interactive-only (3) fusion modes — BUILD
container only.

Runs the unmodified reference model through the existing generators (``run_case`` of make_golden.py,
``model_case`` of make_finetune_golden.py; both import the reference at run time only) in the two
modes the other fixtures do not cover (vilbert_k3m.py:2300-2329, :2388-2402):

* ``golden_bs2_soft.npz``   pretraining step, mode 2 (relu-cat -> sigmoid gate -> soft_* projection);
* ``golden_bs2_inter.npz``  pretraining step, mode 3 ((cross1 + cross2) / 2);
* ``golden_ft_ce_soft.npz`` item-alignment pair step, loss_type ce, mode 2.

Neither mode draws gumbel noise (the recorded ``noise_seed`` is unused, ``noise_order`` is -1).  The two
pretraining cases use 24 region boxes instead of 36: the region features and soft labels are seeded
random floats that do not compress, and 24 boxes keep each fixture under 1 MiB; the fusion under test
is per row and does not depend on the region count.

Usage:  python tests/golden/make_fusion_golden.py [bs2_soft|bs2_inter|ft_ce_soft ...]
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_imports, run_case  # noqa: E402
from make_finetune_golden import model_case  # noqa: E402

CASES = {
    "bs2_soft": lambda: run_case("bs2_soft", row_ids=[13, 17], data_seed=21, weight_seed=61, noise_seed=31,
                                 neg_seed=51, mode=2, R=24),
    "bs2_inter": lambda: run_case("bs2_inter", row_ids=[15, 19], data_seed=22, weight_seed=62, noise_seed=32,
                                  neg_seed=52, mode=3, R=24),
    "ft_ce_soft": lambda: model_case("ce_soft", "ce", 2, row0=160, labels=[0, 1], weight_seed=33, noise_seed=7),
}


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
