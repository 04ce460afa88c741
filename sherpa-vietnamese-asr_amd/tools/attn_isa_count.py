"""Per-key-block instruction counts of the flash attention kernels from their gfx950 assembly
(dev tool; the VALU budget of DESIGN.md §4).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only \
        -S csrc/attn_kernels.hip -o attn.s
  python tools/attn_isa_count.py attn.s [1101 2101 3105 ...]     (MODE NP FMT NF digits)

The key-block loop is unrolled by two (one body per staging register set), so the loop taken is
the shortest backward-branch span that holds two barriers and MFMAs, and every count is halved.
The span includes the paths a block takes only sometimes: the -inf masking of the last key
block (16 v_cmp + 16-17 v_cndmask) and the accumulator rescale when a row maximum moves
(v_pk_mul_f32 of O); `tail_mask` lists the former so that the common path can be read off.
"""
import collections
import re
import sys


def classify(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_exp"):
        return "v_exp"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds_read" if ("read" in op or "load" in op) else "lds_write"
    if op.startswith(("global_load", "buffer_load")):
        return "global_load"
    if op.startswith("s_barrier"):
        return "barrier"
    return "scalar"


def kernels(path: str):
    cur, out = None, {}
    for line in open(path):
        m = re.match(r"^(_ZN4zasr17attn_flash_kernel\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.strip().startswith(".section"):
                cur = None
            else:
                out[cur].append(line)
    return out


def key_block_loop(lines):
    labels, ins = {}, []
    for line in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = line.strip()
        if t and not t.startswith((".", ";")):
            ins.append(t.split(";")[0].strip())
    best = None
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and labels.get(m.group(1), i + 1) <= i:
            body = ins[labels[m.group(1)]:i + 1]
            if (sum(x.startswith("s_barrier") for x in body) == 2 and
                    any(x.startswith("v_mfma") for x in body) and
                    (best is None or len(body) < len(best))):
                best = body
    return best


def main():
    want = sys.argv[2:]
    for name, lines in kernels(sys.argv[1]).items():
        key = "".join(re.search(r"ILi(\d)ELi(\d)ELi(\d)ELi(\d)E", name).groups())
        if want and key not in want:
            continue
        body = key_block_loop(lines)
        if body is None:
            print(key, "no two-barrier key-block loop found")
            continue
        c = collections.Counter(classify(x.split()[0]) for x in body)
        ops = collections.Counter(x.split()[0] for x in body if x.startswith("v_"))
        mask = sum(n for op, n in ops.items() if op.startswith(("v_cmp_gt_i32", "v_cndmask")))
        print(key, "per key block:", {k: v / 2 for k, v in sorted(c.items())}, "tail_mask", mask / 2)
        print("   ", [(op, n / 2) for op, n in ops.most_common(12)])


if __name__ == "__main__":
    main()
