#!/usr/bin/env python3
"""Generate paritytech-bn_amd/csrc/dot2_asm.inc: the hand-scheduled column sum of
fq2_split.h fq_dot2 (REDC(x*y + z*w), nine 29-bit digits, R = 2^261) as one
inline-asm text, and the same for fq_mul (REDC(x*y)) and fq_sqr.

Product scanning with ONE accumulator chain: column k starts from the carry of
column k - 1 (v_lshrrev_b64 by 29) and every digit product of the column is a
v_mad_u64_u32 onto it -- its x*y and z*w products, then m_i * p_(k-i) for the
Montgomery digits already known -- then, for k < 9, m_k = (acc * -p^-1) mod 2^29
(v_mul_lo_u32, v_bfe_u32) and acc += m_k * p_0; for k >= 9 output digit k - 9 is
the low 29 bits.  The compiler's own schedule starts every column as a separate
chain and merges the carry in with a v_lshl_add_u64 (16 per product); a
dependent v_mad_u64_u32 costs no more issue time than an independent one on
gfx950 (profiles/r3j_mad_issue.txt: 9.54 cycles per wave at dep1 and dep8), so
the single chain drops those merges (measured, profiles/r5b_ab_dot2_asm.txt:
k_pairing_full -1.9 %, config 5 -3 %, G2 * Fr -4.4 %, config 3 -5.8 %).  One asm
statement per column instead (C++ between them for m_k and the shifts) drew 1,845
s_nop from the hazard recognizer in k_pairing_full: not used.  The column sums are the compiler form's
(the same terms, the carry added first instead of last), so the value and every
bound are unchanged: m_k depends only on the column's low 29 bits.

Registers: the accumulator is the fixed pair v[2:3] (a clobber: the 32-bit low
half feeds v_mul_lo_u32 / v_bfe_u32, and an asm operand cannot name half of a
64-bit operand); m_k lives in output operand k, whose digit is written only
after m_k's last use (column k + 8 < k + 9).  vcc takes the unused carry-out.
Operands: %0-%8 r (=&v), then x, y[, z, w] (v), then p_0..p_8 and -p^-1 (s).

Addend-taking kinds ('dot2a1' .. 'dot2a3'): the dot2 chain, whose columns 9..17 --
the ones that leave as output digits 0..8, i.e. weight R = 2^261 -- also take digit d
of up to three addend vectors c_j as v_mad_u64_u32 acc, c_j[d], K_j, acc with K_j an
inline constant ("n" operand): r * R == x*y + z*w + R * sum(K_j * c_j) (mod p), so
r == REDC(x*y + z*w) + sum(K_j * c_j) as an integer.  A small multiple and a sum of
terms that would be digit-wise passes and a carry pass after the product cost one
multiply-add per digit here and leave normalized.  Operands: r, x, y, z, w, c_0[,
c_1[, c_2]] (v), p_0..p_8, -p^-1 (s), K_0[, K_1[, K_2]] (n).

One-product kinds with addends ('mula1' .. 'mula3'): the mul chain with the same addend
columns, r == REDC(x*y) + sum(K_j * c_j) (fq2_split.h fq_mul_add: a square whose result
would be followed by additions or subtractions of stored values).  Operands: r, x, y,
c_0[, c_1[, c_2]] (v), p_0..p_8, -p^-1 (s), K_0[, K_1[, K_2]] (n).

Four-product kinds ('dot4', 'dot4a1', 'dot4a2'): REDC(x_0*y_0 + .. + x_3*y_3) [+ sum(K_j *
c_j)], dot6's operand order with four products -- this lane's coordinate of a sum or
difference of two Fq2 products with one reduction (fq2_split.h fq_dot4; the addition
step of the Miller loop).  Operands: r, x_0, y_0, .., x_3, y_3[, c_0[, c_1]] (v), p, -p^-1
(s)[, K_0[, K_1]] (n).

Linear kinds ('lin2', 'lin3'): no product, only the addends -- the normalized digits
of sum(K_j * c_j) as one carry chain (per digit: the carry shift, one multiply-add per
term, the 29-bit extract), for a small-constant combination whose multiples would
overflow 32-bit digits or need a carry pass of their own.  Operands: r, c_0, c_1[,
c_2] (v), K_0, K_1[, K_2] (n).
"""
import os

ACC = "v[2:3]"
ACC_LO = "v2"


def gen(kind):
    """kind: 'dot2' (x*y + z*w), 'dot4' / 'dot6' (sum of four / six products: the addition
    step's merged products, pairing.h's sparse line product), 'mul' (x*y) or 'sqr' (x*x with
    doubled cross terms: d = 2x); 'dot2a<n>', 'dot4a<n>', 'mula<n>': with n addend vectors"""
    if kind.startswith("lin"):
        return gen_lin(int(kind[3:]))
    nadd = 0  # addend vectors at weight R
    for base in ("dot2", "dot4", "mul"):
        if kind.startswith(base + "a"):
            kind, nadd = base, int(kind[len(base) + 1:])
    nprod = {"dot2": 4, "dot4": 8, "dot6": 12, "mul": 2, "sqr": 2}[kind]
    nin = nprod + nadd
    X = lambda i: "%%%d" % (9 + i)                    # noqa: E731
    Y = lambda j: "%%%d" % (18 + j)                   # noqa: E731 (sqr: the doubled digits d)
    Z = lambda i: "%%%d" % (27 + i)                   # noqa: E731
    W = lambda j: "%%%d" % (36 + j)                   # noqa: E731
    pbase = 9 + 9 * nin
    P = lambda j: "%%%d" % (pbase + j)                # noqa: E731
    PINV = "%%%d" % (pbase + 9)
    M = lambda i: "%%%d" % i                          # noqa: E731
    C = lambda t, d: "%%%d" % (9 + 9 * nprod + 9 * t + d)  # noqa: E731 (addend t, digit d)
    KC = lambda t: "%%%d" % (pbase + 10 + t)          # noqa: E731 (its multiplier)
    out = []
    first = True

    def mad(a, b):
        nonlocal first
        out.append("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (ACC, a, b, "0" if first else ACC))
        first = False

    for k in range(17):
        lo, hi = (0, k) if k < 9 else (k - 8, 8)
        if k:
            out.append("v_lshrrev_b64 %s, 29, %s" % (ACC, ACC))
        for i in range(lo, hi + 1):
            j = k - i
            if kind == "sqr":
                if i < j:
                    mad(X(i), Y(j))
                elif i == j:
                    mad(X(i), X(i))
            elif kind in ("dot4", "dot6"):
                for t in range(nprod // 2):  # operands: x_t %(9 + 18t + i), y_t %(18 + 18t + j)
                    mad("%%%d" % (9 + 18 * t + i), "%%%d" % (18 + 18 * t + j))
            else:
                mad(X(i), Y(j))
                if kind == "dot2":
                    mad(Z(i), W(j))
        for i in range(lo, hi + 1):
            if i < k:
                mad(M(i), P(k - i))
        if k < 9:
            out.append("v_mul_lo_u32 %s, %s, %s" % (M(k), ACC_LO, PINV))
            out.append("v_bfe_u32 %s, %s, 0, 29" % (M(k), M(k)))
            mad(M(k), P(0))
        else:
            for t in range(nadd):
                mad(C(t, k - 9), KC(t))
            out.append("v_bfe_u32 %s, %s, 0, 29" % (M(k - 9), ACC_LO))
    out.append("v_lshrrev_b64 %s, 29, %s" % (ACC, ACC))
    for t in range(nadd):
        mad(C(t, 8), KC(t))
    out.append("v_mov_b32 %s, %s" % (M(8), ACC_LO))
    return out


def gen_lin(n):
    out = []
    for d in range(9):
        if d:
            out.append("v_lshrrev_b64 %s, 29, %s" % (ACC, ACC))
        for t in range(n):
            out.append("v_mad_u64_u32 %s, vcc, %%%d, %%%d, %s" % (ACC, 9 + 9 * t + d, 9 + 9 * n + t,
                                                             ACC if d or t else "0"))
        out.append("v_bfe_u32 %%%d, %s, 0, 29" % (d, ACC_LO) if d < 8 else "v_mov_b32 %%8, %s" % ACC_LO)
    return out


KINDS = ("dot2", "mul", "sqr", "dot6", "dot2a1", "dot2a2", "dot2a3", "lin2", "lin3",
         "mula1", "mula2", "mula3", "dot4", "dot4a1", "dot4a2")


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "..", "paritytech-bn_amd", "csrc", "dot2_asm.inc")
    lines = ["// dot2_asm.inc -- GENERATED by tools/gen_dot2_asm.py (do not edit): the single-chain",
             "// column sums of fq_dot2 / fq_mul / fq_sqr (fq2_split.h, fq.h BN_DOT2_ASM) and of the",
             "// six-product sum of the sparse line product (tower.h fq_dot6p); DOT2A<n>: dot2",
             "// with n addend vectors at weight R, LIN<n>: the normalized sum of n small multiples",
             "// (fq2_split.h fq_dot2_add, fq_lin); MULA<n>: mul with n addend vectors,",
             "// DOT4[A<n>]: the four-product sum (fq2_split.h fq_mul_add, fq_dot4; curve.h BN_LINE_CHAIN).",
             "#pragma once"]
    for kind in KINDS:
        ins = gen(kind)
        nmad = sum(1 for s in ins if s.startswith("v_mad"))
        lines.append("// %s: %d instructions, %d v_mad_u64_u32" % (kind, len(ins), nmad))
        lines.append("#define BN_ASM_%s \\" % kind.upper())
        lines += ['    "%s\\n\\t" \\' % s for s in ins[:-1]]
        lines.append('    "%s\\n\\t"' % ins[-1])
    open(dst, "w").write("\n".join(lines) + "\n")
    print("wrote", os.path.normpath(dst))


if __name__ == "__main__":
    main()
