"""Registers, scratch, LDS and waves per SIMD of the kernels that build late anchors and of k_local_cluster, before and after a change, from two build logs:
    make -C scrubby_amd/csrc CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> LOG      (once per tree)
    python scripts/kernel_resources.py BEFORE.log AFTER.log OUT.json
Lists the kernels that lost a wave per SIMD or gained scratch (profiles/late_anchors_resources.json keeps the result); exit status 1 if any.
To be run again after a compiler update: stage_anchors / late_anchors steer the register allocator (two empty asm pins, the kernel-argument
segment) and the class left out in late_class() rests on these figures."""
import json, re, subprocess, sys

KERNELS = r"k_expand<false>|k_sort_top<|k_sort_lds<|k_giant_chunksort|k_local_cluster<"
FIELDS = (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r"    VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
          ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(K[23]Args.*\)$", "", name).replace("void ", "")
            cur = name if re.match(KERNELS, name) else None
            if cur:
                out[cur] = {}
            continue
        if cur:
            for key, pat in FIELDS:
                m = re.search(pat, line)
                if m:
                    out[cur][key] = int(m.group(1))
    return out


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    bad = [k for k in after if k in before and (after[k]["waves_per_simd"] < before[k]["waves_per_simd"] or after[k]["scratch_bytes_per_lane"] > before[k]["scratch_bytes_per_lane"])]
    res = {"source": "hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (the Makefile's flags plus the remark); scripts/kernel_resources.py",
           "rule": "no kernel with fewer waves per SIMD or more scratch than before",
           "kernels": {k: {"before": before.get(k), "after": after[k]} for k in sorted(after)}, "kernels_with_fewer_waves_or_more_scratch": bad}
    json.dump(res, open(sys.argv[3], "w"), indent=1)
    for k in sorted(after):
        print(k, before.get(k), after[k], sep="\n   ")
    print("fewer waves or more scratch:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
