"""Per-kernel table of one depth-network weight-tuning step (`all` mode, N = 6, 640x192) from the kernel_stats.csv of
`rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/depthnet_grad_timing.py --profile-only` (5 steps).  Rows:
every kernel instantiation (time per step); then the families with their useful FLOP per step and TF/s against the 157.3 TF fp32
matrix peak: forward convolutions (k_dn_*: the direct count), data gradients (k_dnb_dgrad: the forward count of every layer but
conv1 and the head), weight gradients (k_dnb_wgrad: the forward count of every convolution but the head).  The others are
memory-bound.
    python scripts/depthnet_grad_kernel_table.py <kernel_stats.csv>   # -> CSV on stdout (profiles/r07_depthnet_grad_kernel_stats.csv)"""
import csv, os, sys
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from depthnet_kernel_table import layers      # (name, multiply-adds per image) of the 640x192 network

N, STEPS, PEAK_TF = 6, 5, 157.3


def main(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_dn" in r["Name"]]
    L = layers()
    mac = dict(L)
    fwd = sum(m for _, m in L)
    fam = {"k_dn_": 2 * fwd * N, "k_dnb_dgrad": 2 * (fwd - mac["conv1+bn1+relu"] - mac["predict_disps.0"]) * N,
           "k_dnb_wgrad": 2 * (fwd - mac["predict_disps.0"]) * N}
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "calls_per_step", "us_per_step", "share_of_step"])
    tot = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / STEPS
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        us = float(r["TotalDurationNs"]) / 1e3 / STEPS
        w.writerow([r["Name"].split("(")[0].replace("void ", "").replace("tc::", ""), int(r["Calls"]) // STEPS, round(us, 1), round(us / tot, 3)])
    w.writerow(["family", "", "us_per_step", "GFLOP_per_step", "TFLOPs", "fraction_of_fp32_matrix_peak"])
    for f, flop in fam.items():
        us = sum(float(r["TotalDurationNs"]) for r in rows if f in r["Name"] and (f != "k_dn_" or "k_dnb_" not in r["Name"])) / 1e3 / STEPS
        tf = flop / 1e9 / us * 1e3 if us else 0.0       # GFLOP per us = PFLOP/s
        w.writerow([f + "*", "", round(us, 1), round(flop / 1e9, 2), round(tf, 1), round(tf / PEAK_TF, 3)])
    w.writerow(["all k_dn* kernels", "", round(tot, 1), "", "", ""])


if __name__ == "__main__":
    main(sys.argv[1])
