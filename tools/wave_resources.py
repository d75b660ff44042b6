"""Registers and scratch of every instance of the two wave-per-cell kernels (csrc/ard_wave.hip, csrc/hyper_wave.hip), read from
the code-object metadata in their gfx950 assembly (tools/check_barriers.py: assemble(), build.sh's flags + -S
--cuda-device-only), and the conditions their __launch_bounds__ set: 128 / 168 / 256 registers per lane for 4 / 3 / 2
workgroups of 256 per CU, and no more scratch than the same instance of a parent checkout, when one is given.

    python tools/wave_resources.py [--parent <csrc directory of a checkout of the parent>] [output.json]
"""
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_barriers as cb  # noqa: E402

TREE = cb.CSRC
FIELDS = (("vgpr", r"\.vgpr_count:\s+(\d+)"), ("sgpr", r"\.sgpr_count:\s+(\d+)"), ("scratch", r"\.private_segment_fixed_size:\s+(\d+)"))


def instances(csrc):
    """{"nlml_wave_kernel<32, 4>": {vgpr, sgpr, scratch, cap}} of the two units under csrc."""
    cb.CSRC, out = csrc, {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("ard_wave", "hyper_wave"):
            for block in open(cb.assemble(unit, tmp)).read().split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                m = re.search(r"(nlml_wave_kernel|hyper_wave_kernel)ILi(\d+)ELi(\d+)(?:ELi(\d+))?E", name)
                if m:
                    nmax, d = int(m.group(2)), int(m.group(3))
                    key = f"{m.group(1)}<{', '.join(g for g in m.groups()[1:] if g)}>"
                    out[key] = {k: int(re.search(rx, block).group(1)) for k, rx in FIELDS}
                    out[key]["cap"] = 256 if nmax > 32 else 168 if d == 16 else 128   # (GPBO_WAVE_BOUNDS of wave_cell.h)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = instances(args[1]) if args[:1] == ["--parent"] else None
    tree = instances(TREE)
    bad = [k for k, v in tree.items() if v["vgpr"] > v["cap"] or (parent and v["scratch"] > parent[k]["scratch"])]
    res = {"instances": len(tree), "violations": bad, "tree": tree}
    if parent:
        res["parent"] = parent
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args[2 if parent else 0:]:
        with open(args[-1], "w") as f:
            f.write(text + "\n")
    sys.exit(1 if bad or len(tree) != 64 else 0)
