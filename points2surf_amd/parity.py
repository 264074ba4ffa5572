"""Comparing an SDF array with a reference one (bench.py's self-check and the full-grid parity tests).

The reference decides the sign as ``sign logit >= 0`` (source/sdf_nn.py:16-21): a query whose sign logit lies within
the fp32 noise of zero (|logit| of a few 1e-6 at a logit accuracy of ~1.5e-5; about 1 query in 400,000) has no
reproducible sign -- the reference itself answers differently for it depending on its batch composition.  Such
queries are compared by magnitude and reported separately; whether a flip really is such a tie is decided by the
caller from the device's own sign logit (engine.query_logits)."""
import numpy as np

# |sign logit| below which a flipped sign counts as a tie of the sign decision, per encoder arithmetic:
#  * IEEE fp32 encoder (cfg.encoder_bf16 = 0): what bounds it is the REFERENCE's own reproducibility -- the same ATen ops on
#    the same network inputs in another batch composition / thread count (oracle/torch_port.py) answer -7.4e-6 for query
#    46,971 of the 512^3 grid of the test shape (p2s_max) where the reference's golden run said >= 0 (r06, found when the
#    parity tests started to demand the CPU port's logit as well as the device's; device: -6.5e-6 with the 16-row tail
#    tile, -4.0e-6 with r05's summation order); 5.0e-6 for the other tie of that grid; at 256^3 the known ties sit at
#    2.4e-7 and 1.7e-6.  The logit accuracy of fp32 through the 1024-wide layers is ~1.5e-5.  1e-5 covers what the
#    reference does to itself and nothing beyond its own noise.  (r02-r05: 6e-6, set from the device's logits alone.)
#  * split-precision encoders (3 bf16 pieces / fp16 pair, 22-24 mantissa bits per operand and another summation order):
#    largest tie seen 8e-6 -> 2e-5, the logit accuracy of those modes.
TIE_LOGIT_FP32 = 1e-5
TIE_LOGIT_SPLIT = 2e-5


def tie_logit(encoder_bf16=0):
    """the tie threshold of an encoder mode (cfg.encoder_bf16: 0 fp32, 3 bf16x3, 4 fp16 pair)"""
    return TIE_LOGIT_FP32 if not encoder_bf16 else TIE_LOGIT_SPLIT


def compare_sdf(sdf, ref):
    """-> dict(max_abs_dsdf, flipped): max |sdf - ref| with the MAGNITUDES compared where the signs differ, and the
    indices of those queries"""
    sdf, ref = np.asarray(sdf), np.asarray(ref)
    if sdf.shape != ref.shape:
        raise ValueError('shape %s vs reference %s' % (sdf.shape, ref.shape))
    flipped = np.nonzero(np.sign(sdf) != np.sign(ref))[0]
    d = np.abs(sdf - ref)
    d[flipped] = np.abs(np.abs(sdf[flipped]) - np.abs(ref[flipped]))
    return {'max_abs_dsdf': float(d.max()) if d.size else 0.0, 'flipped': flipped}


def is_tie(sign_logit_device, sign_logit_cpu, encoder_bf16=0):
    """THE rule for accepting a sign that differs from the reference's golden (bench.py's self-check, the full-grid parity
    tests, the drop-in's tie report): BOTH the device's own sign logit for the query and the CPU restatement's sign logit
    on the same inputs (the same ATen ops as the reference, oracle/torch_port.py -- computed by the caller, this package does
    not import the oracle) lie within the encoder mode's threshold of zero"""
    t = tie_logit(encoder_bf16)
    return abs(float(sign_logit_device)) < t and abs(float(sign_logit_cpu)) < t


def not_ties(sign_logits, encoder_bf16=0):
    """how many of the flipped queries are NOT ties, given the device's sign logits for them and the encoder mode"""
    t = tie_logit(encoder_bf16)
    return int(sum(abs(float(x)) >= t for x in sign_logits))


# Conditioned bound for logits against a float64 evaluation of the same network (the parity tests of the adversarial
# weight sets, synth.STRESS_MODELS): weights that amplify rounding noise (running_var 1e-6, |trans2 - I| ~ 25, sum(q^2) of
# the QSTN quaternion ~ 0.1) make a fixed absolute tolerance either too loose for well-conditioned queries or too tight for
# the others.  The noise of one query is measured instead: the largest deviation from the float64 logits among several fp32
# evaluations that sum in different orders (the reference's own golden, the numpy oracle, the numpy oracle with reversed
# summation order); a result is accepted within COND_FACTOR times that spread plus an absolute floor per encoder mode.
COND_FACTOR = 4.0
COND_FLOOR_FP32 = 1e-5
COND_FLOOR_SPLIT = 2e-5


def conditioned_bound(ref64, fp32_evals, encoder_bf16=0, factor=COND_FACTOR):
    """per-element bound (same shape as ``ref64``) = factor * max_e |e - ref64| + floor of the encoder mode"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    spread = np.zeros_like(ref64)
    for e in fp32_evals:
        spread = np.maximum(spread, np.abs(np.asarray(e, dtype=np.float64) - ref64))
    return factor * spread + (COND_FLOOR_FP32 if not encoder_bf16 else COND_FLOOR_SPLIT)


def conditioned_excess(x, ref64, bound):
    """|x - ref64| / bound per element: <= 1 is within the conditioned bound (NaN where x or ref64 is NaN)"""
    return np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)) / bound
