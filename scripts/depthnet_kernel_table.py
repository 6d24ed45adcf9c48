"""Per-layer table of the depth network from a rocprofv3 --kernel-trace database of `scripts/depthnet_timing.py --profile-only`
(ten N = 5 forwards at 640x192): every forward is the same sequence of 33 launches; the median over the forwards per launch, with the
layer's direct FLOP count and rate.  -> CSV on stdout (profiles/r06_depthnet_kernel_stats.csv).
    python scripts/depthnet_kernel_table.py <rocprofv3 results .db>"""
import csv, os, sqlite3, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depthnet_twin as dt

N, H, W = 5, 192, 640


def layers():
    """(name, multiply-adds per image) in launch order (depthnet_host.h dn_encode / dn_decode)"""
    out = [("conv1+bn1+relu", 64 * 3 * 49 * (H // 2) * (W // 2)), ("maxpool", 0)]
    for p, ci, co, s, ds in dt._blocks():
        sc = {64: 4, 128: 8, 256: 16, 512: 32}[co]
        hw = (H // sc) * (W // sc)
        name = p.replace(dt.ENC, "")
        out.append((name + "conv1", hw * co * ci * 9))
        if ds:
            out.append((name + "downsample", hw * co * ci))
        out.append((name + "conv2+res", hw * co * co * 9))
    for i in range(5):
        hw = (H >> (4 - i)) * (W >> (4 - i))
        out.append((f"depth_upconvs.{i}", hw * 9 * dt.PLANES[i] * dt.PLANES[i + 1]))
        out.append((f"iconvs.{i}", hw * 9 * dt.PLANES[i + 1] ** 2))
    return out + [("feature_convs.0", H * W * 9 * 32 * 8), ("predict_disps.0", H * W * 9 * 8)]


def main(db):
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration, grid_x, grid_y, grid_z, workgroup_x from kernels where name like '%k_dn_%' order by start").fetchall()
    L = layers()
    assert len(rows) % len(L) == 0, (len(rows), len(L))
    fw = len(rows) // len(L)
    w = csv.writer(sys.stdout)
    w.writerow(["launch", "layer", "kernel", "workgroups", "median_us", "min_us", "GFLOP_direct_N5", "TFLOPs", "forwards"])
    tot = 0.0
    for i, (name, mac) in enumerate(L):
        d = sorted(rows[f * len(L) + i][1] / 1e3 for f in range(fw))
        r = rows[i]
        med = d[len(d) // 2]
        tot += med
        gf = 2 * mac * N / 1e9
        kname = r[0].split("(")[0].replace("void tc::", "").replace("tc::", "")
        w.writerow([i, name, kname, (r[2] // r[5]) * r[3] * r[4], round(med, 2), round(d[0], 2), round(gf, 3), round(gf / med * 1e3, 1) if mac else "", fw])
    w.writerow(["sum", "", "", "", round(tot, 1), "", round(2 * sum(m for _, m in L) * N / 1e9, 2), round(2 * sum(m for _, m in L) * N / 1e9 / tot * 1e3, 1), fw])


if __name__ == "__main__":
    main(sys.argv[1])
