"""A/B timing of the image weight gradient's launch pair (wgrad_h2i_group_kernel + wgrad_h2i_reduce_kernel) between two builds of
libdtc_hip.so, and a hash of what they compute.

    python deep-tracking-control_amd/tools/wgrad_h2i_ab.py --libs OLD.so NEW.so [--rounds 3] [--shape 24576 512 512]

Every measurement is a fresh child process that loads ONE library through DTC_LIB (the libraries alternate, OLD first); a child packs
seeded heavy-tailed operands (dZ rows over 1e-8 .. 1, 30 % zero; X rows over 1e-3 .. 1), runs 50 warm-up launches, then times 5 windows
of 400 launch pairs between device events and prints ms per launch pair, the median window and sha256 over dW and db.  The parent
prints the children's lines and, per library, the medians and their spread (profiles/wgrad_image_errors.txt holds one run)."""
import argparse
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def child(tag, M, N, K):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from dtc_amd import h2i, ops
    dev = "cuda:0"
    g = torch.Generator().manual_seed(5)
    dZ = torch.randn(M, N, generator=g) * 10.0 ** (-8 * torch.rand(M, 1, generator=g))
    dZ[torch.rand(M, generator=g) < 0.3] = 0.0
    X = torch.randn(M, K, generator=g) * 10.0 ** (-3 * torch.rand(M, 1, generator=g))
    dW, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    jobs = [(h2i.HImage.from_tensor(dZ.to(dev)), h2i.HImage.from_tensor(X.to(dev)), dW, 0, db)]
    ws = ops.workspace(h2i.wgrad_group_workspace_bytes(jobs, M), dev)
    for _ in range(50):
        h2i.wgrad_group(jobs, M, ws)
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(400):
            h2i.wgrad_group(jobs, M, ws)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 400)
    h = hashlib.sha256(dW.cpu().numpy().tobytes() + db.cpu().numpy().tobytes()).hexdigest()[:16]
    print(f"AB {tag}: ms per launch pair {' '.join(f'{v:.4f}' for v in out)}  median {sorted(out)[2]:.4f}  sha256 {h}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[24576, 512, 512], metavar=("M", "N", "K"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, *a.shape)
    assert a.libs, "--libs OLD.so NEW.so"
    med = {"old": [], "new": []}
    for _ in range(a.rounds):
        for tag, lib in zip(("old", "new"), a.libs):
            env = dict(os.environ, DTC_LIB=os.path.abspath(lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, "--shape", *map(str, a.shape)], env=env,
                               capture_output=True, text=True, timeout=300)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{tag} ({lib}) failed with exit status {r.returncode}:\n{r.stderr[-2000:]}")
            print(line[0], flush=True)
            med[tag].append(float(line[0].split("median ")[1].split()[0]))
    for tag in ("old", "new"):
        m = sorted(med[tag])
        print(f"{tag}: median of medians {1e3 * m[len(m) // 2]:.1f} us, spread {1e3 * m[0]:.1f} .. {1e3 * m[-1]:.1f} us")


if __name__ == "__main__":
    main()
