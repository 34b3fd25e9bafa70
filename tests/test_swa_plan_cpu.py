"""CPU-only: the launch plan of ivl_swa_fwd / ivl_swa_decode_rows_fwd (csrc/swa.hip), observed without a device.

With workspace = NULL a valid ring call that needs a workspace is refused before any launch with IVL_ERR_WORKSPACE, and the
message carries what the plan chose: the KV split count and the bytes of its partials, or the rope pre-pass.  4000 sampled
shapes are held against tests/adversarial.swa_dispatch, the restatement the GPU probes pin launch by launch.  A case is left
out only when the call would launch (one split, no rope pre-pass): there is nothing to refuse."""
import ctypes
import random

import adversarial as adv

FAKE = 4096          # a non-NULL address the checks never dereference
N_CASES = 4000
MAX_SKIPPED = N_CASES // 4

BS = [1, 1, 2, 3, 4, 8]
TS = [1, 2, 3, 4, 5, 8, 33, 40, 64, 65, 128, 130, 256, 300, 512, 1000, 1024, 4096]
HKVS = [1, 2, 4]
GS = [1, 2, 4, 8]
WS = [2, 8, 96, 300, 512, 700, 1024, 4096, 8192]


def _cases():
    rng = random.Random(0)
    for _ in range(N_CASES):
        B, T, Hkv = rng.choice(BS), rng.choice(TS), rng.choice(HKVS)
        yield B, T, Hkv * rng.choice(GS), Hkv, rng.choice(WS), rng.random() < 0.5


def _args(B, T, Hq, Hkv, W, rope):
    from infinitevl_amd._lib import IVL_BF16, SwaArgs
    a = SwaArgs()
    a.q = a.k_new = a.v_new = a.o = a.k_cache = a.v_cache = FAKE
    a.q_sb, a.q_st, a.q_sh = T * Hq * 128, Hq * 128, 128
    a.kn_sb, a.kn_st, a.kn_sh = T * Hkv * 128, Hkv * 128, 128
    a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d = B, T, T, Hq, Hkv, 128
    a.cache_capacity, a.window = W - 1, W
    a.scaling = 1.0
    a.mma_dtype = IVL_BF16
    a.append_new = 1
    if rope:
        a.rope_cos = a.rope_sin = FAKE
        a.rope_s0, a.rope_s1 = 16, 24
    return a                                             # workspace = NULL, workspace_bytes = 0


def _partials_bytes(B, nsplit, T, Hq):
    return B * nsplit * T * Hq * 130 * 4                 # fp32 [B, nsplit, T, Hq, 128 + (m, l)]


def test_swa_fwd_plan_is_the_restated_dispatch():
    from infinitevl_amd import _lib
    lib = _lib.load()
    skipped = 0
    for B, T, Hq, Hkv, W, rope in _cases():
        kern, nsplit = adv.swa_dispatch(B, T, Hq, Hkv, W)
        prepass = rope and kern == "prefill" and (nsplit > 1 or T >= 512)
        if nsplit == 1 and not prepass:
            skipped += 1                                 # the call would launch
            continue
        case = (B, T, Hq, Hkv, W, rope, kern, nsplit)
        rc = lib.ivl_swa_fwd(ctypes.byref(_args(B, T, Hq, Hkv, W, rope)), None)
        msg = lib.ivl_last_error().decode()
        assert rc == _lib.IVL_ERR_WORKSPACE, (case, rc, msg)
        if nsplit > 1:
            assert f"required {_partials_bytes(B, nsplit, T, Hq)} (nsplit={nsplit})" in msg, (case, msg)
        else:
            assert "(rope pre-pass)" in msg, (case, msg)
    assert skipped <= MAX_SKIPPED, skipped               # 858 of 4000 with this seed


def test_decode_rows_plan_is_the_packed_plan_of_swa_fwd():
    from infinitevl_amd import _lib
    lib = _lib.load()
    checked = 0
    for B, T, Hq, Hkv, W, rope in _cases():
        if T * (Hq // Hkv) > 64:
            continue                                     # not packed decode rows: refused as unsupported, no plan
        kern, nsplit = adv.swa_dispatch(B, T, Hq, Hkv, W, rows=True)
        assert kern == "rows" and nsplit > 1 and nsplit == adv.swa_dispatch(B, T, Hq, Hkv, W)[1]
        case = (B, T, Hq, Hkv, W, rope, nsplit)
        rc = lib.ivl_swa_decode_rows_fwd(ctypes.byref(_args(B, T, Hq, Hkv, W, rope)), FAKE, None)
        msg = lib.ivl_last_error().decode()
        assert rc == _lib.IVL_ERR_WORKSPACE, (case, rc, msg)
        assert f"required {_partials_bytes(B, nsplit, T, Hq)} (nsplit={nsplit})" in msg, (case, msg)
        checked += 1
    # 6 of the 18 T values pack at every Hq/Hkv and 3 more at Hq/Hkv = 1: 37.5 % of the draws (1500 of 4000 with this seed)
    assert checked >= N_CASES // 4, checked
