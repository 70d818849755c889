"""Record the sha256 digests of flash_fwd64_kernel's outputs for every launch of tests/attn64_seam_cases.py (needs the GPU):
    VITA_HIP_LIB=/path/to/the/parent/libvita_hip.so python tools/record_attn64_digests.py [OUT.json]
Run it on the build whose bits are to be kept (the commit BEFORE a change of attn64.hip that must not move a bit); the default
destination is tests/golden/attn64_parent_digests.json, which tests/test_attn64_seams_gpu.py demands of the current build.  Every
launch is made twice and must repeat itself, and is checked against fp32 math with the op's own limits before its digest is kept."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import attn64_cases as C  # noqa: E402
import attn64_seam_cases as SC  # noqa: E402
from long_vita_amd import lib, ops  # noqa: E402

lib.load(allow_build=False)
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attn64_parent_digests.json")
digests = {}
for name in SC.NAMES:
    c = SC.case(name)
    out, lse = SC.run(ops, name)
    again = SC.run(ops, name)
    assert torch.equal(out, again[0]) and torch.equal(lse, again[1]), name
    rows = c["rows"] if c["rows"] is not None else (slice(c["empty"].stop, None) if c["empty"] is not None else slice(None))
    err = C.rel_l2(out[:, rows], c["ref"][:, rows])
    assert err <= c["lim"][0], (name, err)
    digests[name] = SC.digests(out, lse)
    print(f"{name}: rel_l2 {err:.3e} o {digests[name]['o'][:16]} lse {digests[name]['lse'][:16]}", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
with open(dst, "w") as f:
    json.dump({"kernel": "flash_fwd64_kernel", "what": "sha256 of the output (bf16) and lse (fp32) bytes per launch of tests/attn64_seam_cases.py",
               "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", dst)
