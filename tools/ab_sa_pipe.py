"""Same-box A/B of the pipelined SA2 scale kernel (csrc/sa_pipe.hip) between builds of the library: one process per build
(CAPTRA_LIB), the builds alternating, two rounds; per build and shape five blocks of 200 back-to-back launches between events at
32 clouds, and a hash of the output (the builds must agree bit for bit).
Usage: python tools/ab_sa_pipe.py parent=/path/to/libcaptra_hip.so change=captra_amd/lib/libcaptra_hip.so [...]"""
import hashlib
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {"sa2s1": (320, (128, 128, 256), 512, 128, 64), "sa2s2": (320, (128, 196, 256), 512, 128, 128)}


def child():
    import torch
    sys.path.insert(0, str(ROOT))
    from captra_amd import fused
    dev = torch.device("cuda:0")
    B = 32
    for name, (cfeat, ch, n, m, k) in SHAPES.items():
        g = torch.Generator(device="cpu").manual_seed(0)
        xyz = (torch.rand(B, 3, n, generator=g) - 0.5).to(dev)
        feat = torch.randn(B, cfeat, n, generator=g).to(dev)
        new_xyz = (torch.rand(B, m, 3, generator=g) - 0.5).to(dev)
        idx = torch.randint(0, n, (B, m, k), generator=g, dtype=torch.int32).to(dev)
        dims = (cfeat + 3,) + ch
        layers = [fused.pack((torch.randn(dims[i], dims[i + 1], generator=g) / dims[i] ** 0.5).to(dev), torch.randn(dims[i + 1], generator=g).to(dev)) for i in range(3)]
        out = torch.empty(B, ch[2], m, device=dev)
        v1 = fused.sa_first_layer_pre_pm(feat, layers[0])
        run = lambda: fused.sa_scale_pre_pm(v1, xyz, new_xyz, idx, layers, out, 0, cfeat)  # noqa: E731
        for _ in range(50):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 200 * 1e3)
        h = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
        print(f"{os.environ.get('TAG')} {name} us/launch blocks {' '.join(f'{t:.1f}' for t in times)}  median {sorted(times)[2]:.1f}  out sha1 {h}", flush=True)


def main():
    libs = {a.split("=", 1)[0]: Path(a.split("=", 1)[1]).resolve() for a in sys.argv[1:]}
    if not libs:
        raise SystemExit(__doc__)
    for rnd in range(2):
        for tag, lib in libs.items():
            env = dict(os.environ, CAPTRA_LIB=str(lib), TAG=f"r{rnd} {tag}")
            r = subprocess.run([sys.executable, __file__, "child"], env=env, timeout=150)
            if r.returncode != 0:
                print(f"{tag}: exit {r.returncode}; stopping", flush=True)
                sys.exit(1)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["child"] else main()
