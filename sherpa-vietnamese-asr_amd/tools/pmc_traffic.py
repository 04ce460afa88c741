"""HBM traffic per launch of a kernel class from two rocprofv3 PMC passes (FETCH_SIZE and
WRITE_SIZE collected separately: together they exceed the gfx950 counter budget).

bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024: FETCH_SIZE / WRITE_SIZE are in KiB, and on
gfx950 FETCH_SIZE reports half the bytes of wide coalesced reads (MI355X_MICROARCH.md, HBM).

  python tools/pmc_traffic.py FETCH.csv WRITE.csv --key "zipformer-68m|greedy_search|1|bf16|3600|enc_gemm"
          [--out profiles/pmc_traffic.json]

Kernel classes: enc_gemm = gemm_bf16_kernel / gemm_f32_kernel with the dense A loader
(template argument ALOAD = 0) and a [N][K] weight operand, the launches Engine::linear /
linear_h make (the NonlinAttention GEMM, EPI_MULAUX, is class attn_nonlin); any other class
name matches kernels whose name contains it; ffn_fused = the fused FeedforwardModule kernels
(bf16 ffn_fused / ffn_wide, f16x3 ffn_wide_h3 but its d = 128 ConvNeXt instance);
attn_apply = attn_flash_kernel modes 1 and 2 (self-attention), attn_nonlin = its mode 3 (the
fused NonlinAttention).  For the two attention classes the record also carries the bytes per
step the launches need (attn_algorithmic_bytes, from the model configuration and the bench's
planned chunk lengths) beside the PMC bytes per step.
"""
import argparse
import csv
import json
import os
import re


def gemm_args(name: str):
    """(kind, template integer args) of a gemm kernel name, demangled or (for instantiations
    with __bf16 arguments, which rocprofv3 leaves mangled) mangled."""
    m = re.search(r"gemm_(bf16|f32)_kernel<([^>]*)>", name)
    if m:
        return m.group(1), [a.strip() for a in m.group(2).split(",")]
    m = re.search(r"gemm_(bf16|f32)_kernelI((?:Li\d+E|Lb[01]E)+)", name)
    if m:
        vals = re.findall(r"L(i|b)(\d+)E", m.group(2))
        return m.group(1), [("false" if v == "0" else "true") if t == "b" else v for t, v in vals]
    return None, None


def _int_args(name: str, kernel: str):
    m = re.search(kernel + r"<([^>]*)>", name)
    return [a.strip() for a in m.group(1).split(",")] if m else None


def in_class(name: str, cls: str) -> bool:
    if cls == "enc_gemm":
        # f16x3 projections: the row-resident kernel, and the dense-A instances of the LDS-DMA
        # and register-tile kernels (ALOAD 0; the others are the subsampling convolutions)
        if "gemm_h3r_kernel" in name:
            return True
        a = _int_args(name, "gemm_glds_h3_kernel")
        if a is not None:
            return a[5] == "0" and a[1] not in ("4", "5")
        a = _int_args(name, "gemm_x3_kernel")
        if a is not None:
            return a[4] == "0" and a[5] not in ("4", "5")
        if "gemm_glds_kernel" in name:  # multi-stage LDS-DMA variant: its EPI_MULAUX(16)
            # z-sliced instances are the NonlinAttention product (class attn_nonlin)
            m = re.search(r"gemm_glds_kernel(?:<\s*\d+,\s*(\d+)|ILi\d+ELi(\d+)E)", name)
            epi = (m.group(1) or m.group(2)) if m else "0"
            return epi not in ("4", "5")
        kind, args = gemm_args(name)
        if kind is None:
            return False
        m = re.match(r"(bf16|f32)", kind)
        if kind == "bf16":
            return args[5] == "0" and args[6] != "4"  # EPI_MULAUX = the NonlinAttention GEMM
        return args[4] == "0" and args[5] == "false"  # B n-contiguous = nonlin_attention

    if cls == "ffn_fused":  # the fused FeedforwardModule launches: bf16 ffn_fused / ffn_wide,
        # f16x3 ffn_wide_h3 except its d = 128 instance (the ConvNeXt MLP, class frontend_conv)
        if "ffn_wide_h3_kernel" in name:
            return "ffn_wide_h3_kernelILi128E" not in name and "ffn_wide_h3_kernel<128" not in name
        return "ffn_wide_kernel" in name or "ffn_fused_kernel" in name
    if cls in ("attn_apply", "attn_nonlin"):
        m = re.search(r"attn_flash_kernel(?:<\s*(\d+)|ILi(\d+)E)", name)
        if not m:
            return False
        mode = int(m.group(1) or m.group(2))
        return mode in (1, 2) if cls == "attn_apply" else mode == 3
    return cls in name


def attn_algorithmic_bytes(cfg, L0, precision: str):
    """Bytes per step that the attention launches need, each operand once per launch.
    L0: encoder frames per chunk at 50 Hz ((fbank frames - 7) // 2); stack i runs its
    num_layers[i] layers on R = sum ceil(L / ds) packed rows.  Element size 2 (bf16) or 4
    (f16x3: f32 storage).
      attn_apply, two launches a layer (modes 1, 2): q / k / p rows [R][68 h] and v rows
        [R][12 h] read, out rows [R][12 h] written, the [R][h] f32 statistics written (mode 1) or
        read (mode 2);
      attn_nonlin, one launch a layer (mode 3): head 0's q / k / p columns [R][68] read,
        t1^T [hid][R32] in bf16 (f16x3: two fp16 images) read, y [R][hid] read, z [R][hid]
        written; hid = 3 d / 4, R32 = sum of L rounded up to 32.
    The positional table (a few hundred KB a layer) is left out."""
    el = 2 if precision == "bf16" else 4
    images = 1 if precision == "bf16" else 2
    apply_b = nonlin_b = 0
    launches = {"attn_apply": 0, "attn_nonlin": 0}
    for d, h, ds, nl in zip(cfg.encoder_dims, cfg.num_heads, cfg.downsampling, cfg.num_layers):
        lens = [-(-L // ds) for L in L0]
        R, R32, hid = sum(lens), sum((L + 31) // 32 * 32 for L in lens), 3 * d // 4
        apply_b += nl * 2 * (R * (68 * h + 2 * 12 * h) * el + R * h * 4)
        nonlin_b += nl * (R * 68 * el + images * hid * R32 * 2 + 2 * R * hid * el)
        launches["attn_apply"] += 2 * nl
        launches["attn_nonlin"] += nl
    return {"attn_apply": apply_b, "attn_nonlin": nonlin_b}, launches


def bench_L0(audio_sec: float, seed: int):
    """The bench's planned chunks (bench.py make_chunks) as encoder frames at 50 Hz."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from zasr.plan import plan_chunks
    from zasr.synth_audio import synth_speech
    audio = synth_speech(audio_sec, seed)
    return [(((e - a) + 80) // 160 - 7) // 2 for a, e, _ in plan_chunks(audio)]


def total(path: str, counter: str, cls: str):
    s, n = 0.0, 0
    with open(path) as f:
        for r in csv.DictReader(f):
            if r["Counter_Name"] == counter and in_class(r["Kernel_Name"], cls):
                s += float(r["Counter_Value"])
                n += 1
    return s, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fetch_csv")
    ap.add_argument("write_csv")
    ap.add_argument("--key", required=True)
    ap.add_argument("--out", default="")
    ap.add_argument("--audio-seed", type=int, default=20261015,
                    help="attention classes: the bench's AUDIO_SEED (planned chunk lengths)")
    a = ap.parse_args()
    cls = a.key.split("|")[-1]
    f, nf = total(a.fetch_csv, "FETCH_SIZE", cls)
    w, nw = total(a.write_csv, "WRITE_SIZE", cls)
    if nf == 0 or nf != nw:
        raise SystemExit("dispatch counts differ or are zero: %d vs %d" % (nf, nw))
    per = (2.0 * f + w) * 1024.0 / nf
    rec = {"bytes_per_launch": round(per), "launches": nf,
           "fetch_kib_x2": round(2 * f), "write_kib": round(w),
           "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), "
                     "FETCH_SIZE x2 gfx950 correction; " + os.path.basename(os.path.dirname(a.fetch_csv))}
    if cls in ("attn_apply", "attn_nonlin"):
        L0 = bench_L0(float(a.key.split("|")[4]), a.audio_seed)  # (puts zasr on the path)
        from zasr.model import zipformer_m, zipformer_s
        model, _, _, precision = a.key.split("|")[:4]
        cfg = {"zipformer-68m": zipformer_m, "zipformer-30m": zipformer_s}[model]()
        alg, per_step = attn_algorithmic_bytes(cfg, L0, precision)
        if nf % per_step[cls]:
            raise SystemExit("%d launches are no whole number of steps (%d a step)" % (nf, per_step[cls]))
        steps = nf // per_step[cls]
        rec["pmc_bytes_per_step"] = round((2.0 * f + w) * 1024.0 / steps)
        rec["algorithmic_bytes_per_step"] = alg[cls]
        rec["pmc_over_algorithmic"] = round(rec["pmc_bytes_per_step"] / alg[cls], 2)
    print(json.dumps({a.key: rec}, indent=1))
    if a.out:
        tab = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                tab = json.load(fh)
        tab[a.key] = rec
        with open(a.out, "w") as fh:
            json.dump(tab, fh, indent=1)


if __name__ == "__main__":
    main()
