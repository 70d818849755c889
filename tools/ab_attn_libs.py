"""Same-box A / B of the forward attention kernel between several builds of the library in ONE process:
    python tools/ab_attn_libs.py [--rounds 7] parent=/path/libvita_hip.so child=/path/libvita_hip.so ...
The first arm is the reference.  Every arm's output at 16K must be bit-identical to the first arm's; then the arms alternate in
interleaved rounds (order reversed every other round), per round the median of 7 / 5 / 3 launches at 16K / 32K / 128K; random
N(0, 1) bf16 inputs, 40 : 8 heads, d = 128, causal.  Prints median, min, max and the rounds per shape and arm (a second copy of the
first build as an arm gives the spread of identical code)."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from long_vita_amd import lib, ops

args = sys.argv[1:]
rounds = 7
if args and args[0] == "--rounds":
    rounds, args = int(args[1]), args[2:]
arms = [a.split("=", 1) for a in args]
handles = {}
for label, path in arms:
    lib._lib, lib.LIB_PATH = None, os.path.abspath(path)
    handles[label] = lib.load(allow_build=False)
    assert isinstance(handles[label], ctypes.CDLL)


def use(label):
    lib._lib = handles[label]


def launch_ms(q, k, v, o, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); ops.flash_attn(q, k, v, causal=True, out=o); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


gen = torch.Generator(device="cuda").manual_seed(0)
first = None
for S, n in ((16384, 7), (32768, 5), (131072, 3)):
    q, k, v = (torch.randn(1, S, h, 128, device="cuda", generator=gen).bfloat16() for h in (40, 8, 8))
    o = torch.empty_like(q)
    if S == 16384:
        for label, _ in arms:
            use(label)
            o.zero_(); ops.flash_attn(q, k, v, causal=True, out=o); torch.cuda.synchronize()
            if first is None:
                first = o.clone()
            else:
                d = (o.float() - first.float())
                print(f"check 16K {label} vs {arms[0][0]}: rel_l2 {float(d.norm() / first.float().norm()):.3e} max_abs {float(d.abs().max()):.3e} "
                      f"equal {torch.equal(o, first)}", flush=True)
                assert torch.equal(o, first), label
    for label, _ in arms:                                  # warm-up of every arm at this shape
        use(label); ops.flash_attn(q, k, v, causal=True, out=o)
    torch.cuda.synchronize()
    res = {label: [] for label, _ in arms}
    for r in range(rounds):
        for label, _ in (arms if r % 2 == 0 else arms[::-1]):
            use(label)
            res[label].append(launch_ms(q, k, v, o, n))
    for label, _ in arms:
        x = res[label]
        med = statistics.median(x)
        print(f"S={S} {label}: median {med:.3f} min {min(x):.3f} max {max(x):.3f} ms over {rounds} rounds "
              f"({4 * 128 * 40 * S * (S + 1) / 2 / med / 1e9:.0f} TF)  rounds: " + " ".join(f"{t:.3f}" for t in x), flush=True)
    del q, k, v, o
print("done")
