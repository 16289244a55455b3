"""Record what the library's host-only queries answer - which kernel a descriptor takes, how large the buffers sized by that choice
are - for a fixed list of descriptors and switch settings, into tests/host_dispatch_expected.py. No GPU is touched.

    LFI_LIB_PATH=<liblfi_hip.so of the commit to pin> python tools/record_host_dispatch.py --commit <its hash>

tests/test_host_dispatch_cpu.py asserts that the library in the tree gives every recorded answer, so the table is recorded from a build
of the commit whose behaviour is to be kept, not from the code under test. Every switch setting is recorded in a fresh child process: a
library that caches a switch at its first call would otherwise answer for the setting it saw first."""
import argparse
import ctypes as C
import json
import os
import pprint
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "host_dispatch_expected.py")

SWITCHES = [
    {},
    {"LFI_ENC_WIDE": "0"}, {"LFI_ENC_WIDE_BWD": "0"}, {"LFI_ENC_R64": "0"}, {"LFI_ENC_M16": "0"}, {"LFI_ENC_T16": "0"}, {"LFI_ENC_T16": "2"},
    {"LFI_FLOW_GENERIC": "1"}, {"LFI_FLOW_PIPE": "0"}, {"LFI_PIPE_X3": "0"}, {"LFI_INVERT_WALK": "0"},
    {"LFI_SAMPLE_CHAIN": "0"}, {"LFI_SAMPLE_WFRAG16": "0"},
]
SWITCH_NAMES = sorted({k for s in SWITCHES for k in s})

# lfi_enc_desc: B, T, N, start, hist, hid, ldcond, col, precision, dup, lstm, bwd_two_products, stash_f16
_HEADLINE_ENCODERS = {   # hparams/final_model_synthetic.yaml at batch 256, T 80: (hist, hid, col) in the 896-wide cond rows
    "p2_face": (24, 256, 256), "p2_speech": (16, 256, 512), "p1_speech": (2, 128, 768)}


def enc_descs():
    out = [("big", (256, 80, 56, 24, 24, 256, 896, 256, 1, 0, 0, 1, 1)),        # the three of test_window_encoder_forward_variant_selection
           ("small", (256, 80, 56, 24, 2, 128, 896, 768, 1, 0, 0, 1, 1)),
           ("ragged", (40, 80, 56, 24, 24, 256, 896, 256, 1, 0, 0, 1, 1))]
    for name, (hist, hid, col) in _HEADLINE_ENCODERS.items():
        for two in (0, 1):
            for f16 in (0, 1):
                out.append(("%s two=%d f16=%d" % (name, two, f16), (256, 80, 56, 24, hist, hid, 896, col, 1, 0, 0, two, f16)))
        out.append((name + " precision 0", (256, 80, 56, 24, hist, hid, 896, col, 0, 0, 0, 0, 0)))
        out.append((name + " lstm", (256, 80, 56, 24, hist, hid, 896, col, 1, 0, 1, 1, 0)))
        out.append((name + " ldcond 898", (256, 80, 56, 24, hist, hid, 898, col, 1, 0, 0, 1, 1)))
    out.append(("hid 320 (unfused)", (256, 80, 56, 24, 24, 320, 896, 256, 1, 0, 0, 1, 0)))
    out.append(("hid 130", (256, 80, 56, 24, 24, 130, 896, 256, 1, 0, 0, 1, 1)))
    return out


# lfi_flow_dims: B, N, C, H, D, Ks, affine, lstm, scale_eps, gemm_precision
_FLOW_SHAPES = [
    ("headline", (256, 56, 50, 128, 512, 16, 1, 0)), ("C 56", (256, 56, 56, 128, 512, 16, 1, 0)),
    ("tiny", (4, 16, 16, 32, 32, 2, 1, 0)), ("odd", (6, 8, 15, 24, 40, 4, 1, 0)), ("mid", (8, 4, 50, 44, 48, 3, 1, 0)),   # tests/golden fixtures
    ("lstm", (256, 56, 50, 128, 512, 16, 1, 1)), ("H 256", (256, 56, 50, 256, 512, 16, 1, 0)),
    ("B 16", (16, 56, 50, 128, 512, 16, 1, 0)), ("B 40", (40, 56, 50, 128, 512, 16, 1, 0))]
_GEMM_PRECISIONS = [0, 1, 5, 9, 1 | (1 << 16)]


def flow_dims():
    return [("%s gemm_precision %#x" % (name, gp), shape + (1e-4, gp)) for name, shape in _FLOW_SHAPES for gp in _GEMM_PRECISIONS]


ENC_QUERIES = ["fwd_variant m0 s0", "fwd_variant m1 s0", "fwd_variant m0 s1", "fwd_variant m1 s1", "bias_rows", "grad_stash_bf16",
               "stash_f16_ok", "compact_dgi", "work_floats"]
FLOW_QUERIES = ["bwd_emits_planes", "seq_rev_ok", "prep_floats", "stash_floats", "bstash_floats", "param_grads_work_floats",
                "seq_rev_work_floats", "sample_work_floats", "sample_nll_work_floats", "frame_plan"]


def enc_answers(L, desc):
    from lets_face_it_amd._lib import EncDesc
    d = C.byref(EncDesc(*desc))
    return [L.lfi_encode_windows_fwd_variant(d, m, s) for s in (0, 1) for m in (0, 1)] + [
        L.lfi_encode_windows_bias_rows(d), L.lfi_encode_windows_grad_stash_bf16(d), L.lfi_encode_windows_stash_f16_ok(d),
        L.lfi_encode_windows_compact_dgi(d), L.lfi_encode_windows_work_floats(d)]


def flow_answers(L, dims):
    from lets_face_it_amd._lib import FlowDims
    d = C.byref(FlowDims(*dims))
    return [L.lfi_flow_bwd_emits_planes(d), L.lfi_flow_seq_rev_ok(d), L.lfi_flow_prep_floats(d), L.lfi_flow_stash_floats(d),
            L.lfi_flow_bstash_floats(d), L.lfi_flow_param_grads_work_floats(d), L.lfi_flow_seq_rev_work_floats(d),
            L.lfi_flow_sample_work_floats(d), L.lfi_flow_sample_nll_work_floats(d), L.lfi_flow_frame_plan(d)]


def answers(L):
    """Every query for every descriptor, under the switches of the current environment."""
    return {"enc": [enc_answers(L, desc) for _, desc in enc_descs()], "flow": [flow_answers(L, dims) for _, dims in flow_dims()]}


def _child():
    sys.path.insert(0, ROOT)
    from lets_face_it_amd import _lib
    print(json.dumps(answers(_lib.lib())))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the commit the library in LFI_LIB_PATH was built from")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child()
    table = []
    for sw in SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in SWITCH_NAMES}
        env.update(sw)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--commit", args.commit, "--child"], env=env, check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        table.append(json.loads(out.strip().splitlines()[-1]))
    with open(OUT, "w") as f:
        f.write('"""Answers of the library\'s host-only queries (which kernel a descriptor takes, the sizes that follow from it), recorded by\n'
                'tools/record_host_dispatch.py from a build of commit %s, for tests/test_host_dispatch_cpu.py. Generated: do not edit;\n'
                'EXPECTED[i] was recorded in a fresh process under SWITCHES[i], one row of answers per descriptor, one answer per query."""\n'
                % args.commit)
        f.write("COMMIT = %r\n" % args.commit)
        for name, value in (("SWITCHES", SWITCHES), ("ENC_QUERIES", ENC_QUERIES), ("FLOW_QUERIES", FLOW_QUERIES), ("ENC_DESCS", enc_descs()),
                            ("FLOW_DIMS", flow_dims()), ("EXPECTED", table)):
            f.write("%s = %s\n" % (name, pprint.pformat(value, width=160, compact=True)))
    print("wrote %s: %d switch settings x (%d encoder descriptors, %d flow dims)" % (OUT, len(SWITCHES), len(enc_descs()), len(flow_dims())))


if __name__ == "__main__":
    main()
