"""Reads the kernel-resource remarks of one compile (hipcc -Rpass-analysis=kernel-resource-usage, stderr kept in a file),
prints what is not a remark (warnings), and checks the instantiations of sfk::view_march_kernel (docs/SPEC.md §13) and
sfk::camera_march_kernel (§14) against the limits of §13: no scratch, no LDS, no AGPRs, at most 128 VGPRs (four waves
per SIMD resident), and the masked kernels of §15 to §19 against theirs: no scratch, no LDS, no AGPRs. Prints their
table."""
import re
import sys

GATHER_KERNELS = ("view_march_kernel", "camera_march_kernel")

LIMITS = {"VGPRs": 128, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 0, "VGPRs Spill": 0}
# the kernels of solid obstacles (docs/SPEC.md §15): row kernels next to unmasked siblings, held to the same absence of
# scratch, AGPRs and LDS (their VGPRs are printed, not capped)
MASKED_KERNELS = ("face_code_kernel", "cg_init_masked_kernel", "cg_apply_dot_masked_kernel", "project_div_masked_kernel",
                  "project_sub_masked_kernel", "zero_solid_kernel",
                  # the V-cycle under a mask (§16)
                  "mg_coarsen_mask_kernel", "mg_smooth_masked_kernel", "mg_restrict_masked_kernel",
                  "mg_prolong_masked_kernel",
                  # mask-aware transport (§17)
                  "lin_solve_masked_kernel", "advect_masked_kernel",
                  # MacCormack under the mask (§18)
                  "advect_mc_masked_kernel",
                  # moving solids (§19): siblings of the two project halves, the sweep and the advect
                  "project_div_moving_kernel", "project_sub_moving_kernel", "lin_solve_moving_kernel",
                  "advect_moving_kernel")
MASKED_LIMITS = {k: v for k, v in LIMITS.items() if k != "VGPRs"}


def main(path):
    kernels, cur, other, skip = {}, None, [], 0
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if m:
            skip = 2  # the source line and the caret that follow a remark
            name = re.match(r"Function Name: (\S+)", m.group(1))
            if name:
                cur = kernels.setdefault(name.group(1), {})
            elif cur is not None and ":" in m.group(1):
                k, v = m.group(1).rsplit(":", 1)
                cur[k.strip()] = v.strip()
        elif skip and not re.match(r"\S+:\d+:\d+: ", line):
            skip -= 1
        else:
            other.append(line)
    other = [ln for ln in other if not ln.startswith("In file included from")]
    sys.stderr.writelines(ln for ln in other if not re.match(r"\d+ (warning|remark)s? generated", ln.strip()) or "warning" in ln)
    bad = 0
    for names, limits in ((GATHER_KERNELS, LIMITS), (MASKED_KERNELS, MASKED_LIMITS)):
        view = {k: v for k, v in kernels.items() if any(name in k for name in names)}
        for name in names:
            if not any(name in k for k in view):
                sys.exit(f"{path}: no {name} among {len(kernels)} kernels")
        for name, r in sorted(view.items()):
            print(f"  {name}: VGPRs {r.get('VGPRs')} AGPRs {r.get('AGPRs')} SGPRs {r.get('TotalSGPRs')} scratch "
                  f"{r.get('ScratchSize [bytes/lane]')} LDS {r.get('LDS Size [bytes/block]')} waves/SIMD "
                  f"{r.get('Occupancy [waves/SIMD]')}")
            for key, cap in limits.items():
                if key not in r or int(r[key]) > cap:
                    print(f"    {key} = {r.get(key)} exceeds {cap}", file=sys.stderr)
                    bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main(sys.argv[1])
