"""Are the kernels of one gfx950 assembly file unchanged in another? For a change that must leave
existing kernels alone: compile csrc/elastic_kernels.hip of both commits with

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -fopenmp --cuda-device-only -S -o X.s ...

(once more with -DAA_LBFGS_RHO=0) and run `python tools/kernel_text_diff.py old.s new.s`. Every
kernel of old.s must have a kernel in new.s with the same instruction text (comments, block labels
and the kernel's own symbol name aside) and the same descriptor: VGPRs, AGPR offset, SGPRs, scratch,
LDS, kernel-argument size. A kernel whose mangled name changed (a template parameter was added) is
matched by text among the new file's kernels of the same function name. Exit status 1 if any differs.
"""
import re
import sys

DESC = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_size")


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        out[m.group(1)] = [m.group(2), {}]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        if m.group(1) in out:
            out[m.group(1)][1] = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
    return {k: v for k, v in out.items() if v[1]}


def text(body, name):
    body = body.replace(name, "K")
    body = re.sub(r";.*", "", body)
    body = re.sub(r"\.?L?BB\d+_", "B_", body)
    body = re.sub(r"\.L\w+", "L", body)
    return re.sub(r"[ \t]+\n", "\n", body)


def function_name(mangled):   # ..._GLOBAL__N_1<len><name>I... -> <name>
    m = re.search(r"GLOBAL__N_1(\d+)(k_\w+)", mangled)
    return m.group(2)[:int(m.group(1))] if m else mangled


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    same, renamed, bad, hits = 0, [], [], set()
    for name, (body, desc) in sorted(old.items()):
        cands = [name] if name in new else [k for k in new if k not in old and function_name(k) == function_name(name)]
        match = [k for k in cands if text(new[k][0], k) == text(body, name)]
        hit = next((k for k in match if k not in hits), match[0] if match else None)   # an unclaimed one first
        if hit is None:
            bad.append(f"{name}: no kernel with this text ({len(cands)} candidates)")
            continue
        diff = [(k, desc.get(k), new[hit][1].get(k)) for k in DESC if desc.get(k) != new[hit][1].get(k)]
        if diff:
            bad.append(f"{name}: descriptor differs {diff}")
            continue
        same += 1
        hits.add(hit)
        if hit != name:
            renamed.append((name, hit))
    print(f"{len(old)} kernels in {old_path}, {len(new)} in {new_path}: {same} unchanged "
          f"({len(renamed)} under a new name, {same - len(hits)} sharing a kernel with another), {len(bad)} changed, "
          f"{len(set(new) - hits)} new")
    for a, b in renamed:
        print("  renamed", a, "->", b)
    for b in bad:
        print("  CHANGED", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
