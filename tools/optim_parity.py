"""Records the parity figures of the native optimizer step (stabletts_amd.optim.AdamW) on an MI355X: the error of the native
update and of torch.optim.AdamW(foreach=False) in fp32 against the float64 restatement (tests/optim_restatement.py), per kind
(p, exp_avg, exp_avg_sq) as max-abs over the concatenation of the list / max-abs of the truth, and their ratio (bar 4), for the
cases of tests/test_gpu_optim.py: the parity list over three steps and the launch-boundary lists.

    python tools/optim_parity.py > profiles/optim_parity.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from tests import test_gpu_optim as T
    C, M = T._cm()
    print(f"# python tools/optim_parity.py   (one MI355X; chunk C = {C}, tensors per launch M = {M})")
    print("# error = max-abs over the concatenation of a list's tensors of a kind / max-abs of the float64 truth; ratio = native / torch fp32 (bar 4)")
    with torch.no_grad():
        e_native, e_torch, steps, _ = T.parity_case()
        T._gate("parity list, 3 steps, 2 groups", e_native, e_torch)
        print(f"parity list: step counters {steps} (tensor 2 had no gradient at step 2)")
        small = T.make_small_tensors()
        for which, length in (("M-1", M - 1), ("M", M), ("M+1", M + 1), ("2M+3", 2 * M + 3)):
            _, e_native, e_torch, _ = T.boundary_case(small, length)
            T._gate(f"list of {which} = {length} tensors of 1..300 elements", e_native, e_torch)


if __name__ == "__main__":
    main()
