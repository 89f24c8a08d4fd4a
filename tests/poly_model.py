"""Big-integer references for the polynomial-stage kernels (algoplonk_amd/csrc/kernels_poly.h), reached one stage at a time
through apk_device_poly_op (include/apk.h).

Two kinds of model, both over STORED WORDS (the 256-bit integers a vector holds; a word w in gnark's radix stands for the field
element w / R mod r, and a semi-canonical word may be anywhere below 2 r):

  * plain references (`ref_*`): the prover's formulas mod r - the grand product, the quotient numerator over Z_H, Horner sums,
    (f - f(z)) / (X - z) ... as SURVEY.md App. E and the kernels' header comments cite them - evaluated on the elements the words
    stand for and returned as the canonical words the kernel must write.  Nothing here follows the kernels' code.
  * value-level models (`lazy_*`) of the kernels that multiply on unsaturated limbs without reducing (GpTermsK, QuotientK,
    subcoset_merge_kernel, EvalPartialK, LincombK, DerivePowersK), in the manner of limb_model.lazy_ntt: mul_nr is its true value
    (a b + m r) / R', sums and k r - b differences are plain integers.  Every named intermediate is recorded with the bound its
    comment states, and three things are checked along the way (a Trace collects what fails, naming the kernel's line):
      - an operand enters in the class the comment gives (below 2 r for l, r, o, z, zs, pi2; below r for tables and challenges);
      - the comment's figure follows from its operands' figures by the header's rule - a product of operands below A r and C r is
        below (1 + A C / 64) r, A C <= 64 - so an operand one class wider than the comment says fails whatever its value;
      - the value itself is below the stated bound, the subtrahend of sub_k<K> is at most K r, and what enters canon<1> /
        reduce_2p<K> is below 2 r / 2 K r.
"""
from __future__ import annotations

from dataclasses import dataclass, field as dc_field
from fractions import Fraction
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

R_BITS, RP_BITS = 256, 261          # gnark's radix R = 2^256; the limb form's R' = 2^(9 x 29) = 32 R (both curves' Fr)
H_MIN = 64                          # the HEADROOM every lazy kernel asserts; the comments' figures are for it
SCAN_BLOCK, POLY_THREADS, EVAL_BLOCK = 2048, 256, 2048
EVAL_MAX, LC_MAX, QK_INJECT_MAX = 12, 20, 6


@lru_cache(maxsize=None)
def _inverse(x: int, m: int) -> int:
    return pow(x, -1, m)


@dataclass(frozen=True)
class Radix:
    """x held as the word x * scale * R mod r.  The ONE place each scale factor of the kernels' headers is written."""
    r: int
    scale: int

    def enc(self, x: int) -> int:
        return x * self.scale % self.r * (1 << R_BITS) % self.r

    def dec(self, w: int) -> int:
        return w * _inverse(self.scale << R_BITS, self.r) % self.r


@dataclass(frozen=True)
class PolyField:
    r: int

    @property
    def Rp(self) -> int:
        return 1 << RP_BITS

    # "x in gnark's radix": polynomial values, gamma, results
    @property
    def gnark(self) -> Radix:
        return Radix(self.r, 1)

    # "x in the product's radix R' = 32 R": what multiplies a value (beta, beta u, zh_inv, inj_delta, coefficients, twiddles)
    @property
    def prod(self) -> Radix:
        return Radix(self.r, 1 << (RP_BITS - R_BITS))

    # "selector tables as the setup scales them": 32 q, and 1024 q for qm (its operand l r is a product of two values)
    @property
    def sel(self) -> Radix:
        return Radix(self.r, 32)

    @property
    def sel_qm(self) -> Radix:
        return Radix(self.r, 32 * 32)

    # alpha has three value products behind it, alpha^2 one
    @property
    def alpha(self) -> Radix:
        return Radix(self.r, 32 ** 4)

    @property
    def alpha2(self) -> Radix:
        return Radix(self.r, 32 ** 2)

    def mont(self, a: int, b: int) -> int:
        """Fe's product of two canonical words: a b / R mod r"""
        return a * b * _inverse(1 << R_BITS, self.r) % self.r


# ---- plain references ----------------------------------------------------------------------------------------------------------
def ref_gp(F: PolyField, L, R, O, S1, S2, S3, tw, beta32, gamma, beta_u32, beta_u2_32):
    """Z[0] = 1, Z[k] = prod_{i<k} num_i / den_i, num_i = prod_j (w_j[i] + beta u^j omega^i + gamma), den_i = prod_j (w_j[i] +
    beta S_j[i] + gamma); the rows' num and den come back divided by 1024 (two value x value products each).  Words in, words
    out.  tw = omega^i for i < n / 2 in gnark's radix; the challenges in the product's radix, gamma in gnark's."""
    r, g, n = F.r, F.gnark, len(L)
    b, bu, bu2, gm = F.prod.dec(beta32), F.prod.dec(beta_u32), F.prod.dec(beta_u2_32), g.dec(gamma)
    om = [g.dec(w) for w in tw]
    om = om + [(r - x) % r for x in om]
    inv1024 = pow(1024, -1, r)
    num, den = [], []
    for i in range(n):
        l, rr, o = g.dec(L[i]), g.dec(R[i]), g.dec(O[i])
        num.append((l + b * om[i] + gm) * (rr + bu * om[i] + gm) % r * (o + bu2 * om[i] + gm) % r)
        den.append((l + b * g.dec(S1[i]) + gm) * (rr + b * g.dec(S2[i]) + gm) % r * (o + b * g.dec(S3[i]) + gm) % r)
    z, acc = [1], 1
    for i in range(n - 1):
        if 0 in den:          # Z is not defined (the caller excludes such inputs; the rows' terms still are)
            z = None
            break
        acc = acc * num[i] % r * pow(den[i], -1, r) % r
        z.append(acc)
    return [g.enc(x * inv1024) for x in num], [g.enc(x * inv1024) for x in den], z and [g.enc(x) for x in z]


def ref_scan(F: PolyField, data: Sequence[int], mul: bool, rev: bool, shift: int) -> List[int]:
    """inclusive prefix (rev: suffix) products / sums of canonical words as Fe computes them; shift: out[0] = identity,
    out[i] = inclusive[i - 1]"""
    r, rinv = F.r, _inverse(1 << R_BITS, F.r)
    src = list(reversed(data)) if rev else list(data)
    out, acc = [], None
    for w in src:
        acc = w if acc is None else (acc * w * rinv % r if mul else (acc + w) % r)
        out.append(acc)
    if shift:
        out = [F.gnark.enc(1) if mul else 0] + out[:-1]
    return list(reversed(out)) if rev else out


def ref_quotient(F: PolyField, q: dict) -> List[int]:
    """The whole 4n coset: (gate + alpha (Z(wX) prod(w_j + beta S_j + gamma) - Z(X) prod(w_j + beta u^j X + gamma)) + alpha^2 L_0
    (Z - 1)) / Z_H at every point i, Z(wX) = z[(i + 4) mod n4].  `q` holds WORDS under QuotientArgs' names, over the whole coset:
    l r o z (gnark, possibly semi-canonical), pi2[k], the tables, the constants - each in the encoding the kernel's header gives."""
    r, g, P = F.r, F.gnark, F.prod
    n4 = len(q["l"])
    al, al2 = F.alpha.dec(q["alpha"]), F.alpha2.dec(q["alpha2"])
    b, bu, bu2, gm = P.dec(q["beta"]), P.dec(q["beta_u"]), P.dec(q["beta_u2"]), g.dec(q["gamma"])
    zh = [P.dec(w) for w in q["zh_inv"]]
    delta = [P.dec(w) for w in q["inj_delta"]]
    out = []
    for i in range(n4):
        l, rr, o, z = (g.dec(q[k][i]) for k in ("l", "r", "o", "z"))
        zs = g.dec(q["z"][(i + 4) % n4])
        gate = (F.sel.dec(q["ql"][i]) * l + F.sel.dec(q["qr"][i]) * rr + F.sel_qm.dec(q["qm"][i]) * l * rr + F.sel.dec(q["qo"][i]) * o
                + g.dec(q["qk"][i]))
        for k in range(q["nb_commit"]):
            gate += F.sel.dec(q["qcp"][k][i]) * g.dec(q["pi2"][k][i])
        for j in range(q["nb_inject"]):
            gate += delta[j] * g.dec(q["inj_tab"][j][i])
        x = g.dec(q["x"][i])
        pa = zs * (l + gm + b * g.dec(q["s1"][i])) % r * (rr + gm + b * g.dec(q["s2"][i])) % r * (o + gm + b * g.dec(q["s3"][i])) % r
        pb = z * (l + gm + b * x) % r * (rr + gm + bu * x) % r * (o + gm + bu2 * x) % r
        loc = al2 * g.dec(q["l0"][i]) % r * (z - 1) % r
        out.append(g.enc(zh[i & 3] * ((gate + al * (pa - pb) + loc) % r)))
    return out


def ref_merge(F: PolyField, part: Sequence[int], post: Sequence[int], rho_inv: Sequence[int], m: int, G: int) -> List[int]:
    """h[c' + m t] = post[c' + m t] * sum_k rho^(-k t) part[k][c'];  post and rho_inv[e] = rho^-e in the product's radix"""
    g, P = F.gnark, F.prod
    rho = [P.dec(w) for w in rho_inv]
    out = [0] * (G * m)
    for t in range(G):
        for cp in range(m):
            s = sum((rho[(k * t) % G] if (k * t) % G else 1) * g.dec(part[k * m + cp]) for k in range(G))
            out[t * m + cp] = g.enc(P.dec(post[t * m + cp]) * s)
    return out


def ref_eval(F: PolyField, f: Sequence[int], pw: Sequence[int]) -> int:
    """sum_i f[i] pw[i] / 32: both operands are values in gnark's radix"""
    g = F.gnark
    return g.enc(sum(g.dec(a) * g.dec(b) for a, b in zip(f, pw)) * pow(32, -1, F.r))


def ref_lincomb(F: PolyField, fs: Sequence[Sequence[int]], coef32: Sequence[int], out_len: int) -> List[int]:
    g, P = F.gnark, F.prod
    cs = [P.dec(c) for c in coef32]
    return [g.enc(sum(c * g.dec(f[i]) for c, f in zip(cs, fs) if i < len(f))) for i in range(out_len)]


def ref_derive(F: PolyField, vin: Sequence[int], twu: Sequence[int], n: int, inverse: int) -> List[int]:
    """out[i] = in[i] * omega^(+-i); twu[j] = omega^j in the product's radix, j < n / 2, omega^(n/2) = -1"""
    g, r = F.gnark, F.r
    om = [F.prod.dec(w) for w in twu]
    om = om + [(r - x) % r for x in om]
    return [g.enc(g.dec(v) * om[(-i if inverse else i) % n]) for i, v in enumerate(vin)]


def ref_kzg_quotient(F: PolyField, f: Sequence[int], z: int) -> List[int]:
    """(f - f(z)) / (X - z) by synthetic division: q[len-2] = f[len-1], q[j-1] = f[j] + z q[j].  f in words, z an element."""
    g, r = F.gnark, F.r
    c = [g.dec(w) for w in f]
    q = [0] * (len(c) - 1)
    acc = 0
    for j in range(len(c) - 1, 0, -1):
        acc = (c[j] + z * acc) % r
        q[j - 1] = acc
    return [g.enc(x) for x in q]


def ref_blind(F: PolyField, p: Sequence[int], n: int, b: Sequence[int], d: int) -> List[int]:
    """p(X) += b(X) (X^n - 1), deg b = d - 1: p[i] -= b[i], p[n + i] = b[i] (assigned).  Canonical words: Fe's sub is on words."""
    out = list(p)
    for i in range(d):
        out[i] = (p[i] - b[i]) % F.r
        out[n + i] = b[i]
    return out


# ---- value-level models ----------------------------------------------------------------------------------------------------------
@dataclass
class LV:
    v: int                 # the value the limbs hold
    ub: Fraction           # what the comments' rule gives for it, in units of r (exclusive)


@dataclass
class Trace:
    F: PolyField
    kernel: str
    named: Dict[str, Tuple[int, float]] = dc_field(default_factory=dict)     # intermediate -> (value, stated bound in r)
    bad: List[str] = dc_field(default_factory=list)

    def _say(self, line: str, what: str) -> None:
        self.bad.append("%s, line `%s`: %s" % (self.kernel, line, what))

    def operand(self, name: str, w: int, cls: int, line: str) -> LV:
        if not 0 <= w < cls * self.F.r:
            self._say(line, "%s enters at %.4f r, the comment takes it below %d r" % (name, w / self.F.r, cls))
        return LV(w, Fraction(cls))

    def stated(self, name: str, x: LV, bound, line: str) -> LV:
        """the comment's figure for a named intermediate: it must follow from the operands' figures, and hold for the value"""
        bound = Fraction(bound)
        self.named[name] = (x.v, float(bound))
        if x.ub > bound:
            self._say(line, "%s: the operands' classes give %.4f r, the comment states %.4f r" % (name, float(x.ub), float(bound)))
        if not x.v < bound * self.F.r:
            self._say(line, "%s = %.4f r is not below the stated %.4f r" % (name, x.v / self.F.r, float(bound)))
        return LV(x.v, min(x.ub, bound))

    def mul_nr(self, a: LV, b: LV, line: str) -> LV:
        F = self.F
        if a.ub * b.ub > H_MIN:
            self._say(line, "mul_nr of operands below %.3f r and %.3f r: their product exceeds the headroom %d" % (float(a.ub), float(b.ub), H_MIN))
        t = a.v * b.v
        m = t * (-_inverse(F.r, F.Rp) % F.Rp) % F.Rp
        return LV((t + m * F.r) // F.Rp, 1 + a.ub * b.ub / H_MIN)

    @staticmethod
    def add_n(a: LV, b: LV) -> LV:
        return LV(a.v + b.v, a.ub + b.ub)

    def sub_k(self, K: int, a: LV, b: LV, line: str) -> LV:
        if b.ub > K or not b.v <= K * self.F.r:
            self._say(line, "sub_k<%d>: the subtrahend (%.4f r, class %.4f r) may exceed %d r" % (K, b.v / self.F.r, float(b.ub), K))
        return LV(a.v - b.v + K * self.F.r, a.ub + K)

    def reduce_2p(self, K: int, a: LV, line: str) -> LV:
        if a.ub > 2 * K or not a.v < 2 * K * self.F.r:
            self._say(line, "reduce_2p<%d> takes values below %d r, got %.4f r (class %.4f r)" % (K, 2 * K, a.v / self.F.r, float(a.ub)))
        return LV(a.v % self.F.r, Fraction(2))      # some representative below 2 r: only its residue goes on

    def canon1(self, a: LV, line: str) -> int:
        if a.ub > 2 or not a.v < 2 * self.F.r:
            self._say(line, "canon<1> takes values below 2 r, got %.4f r (class %.4f r)" % (a.v / self.F.r, float(a.ub)))
        return a.v % self.F.r


def lazy_gp_terms(F: PolyField, L, R, O, S1, S2, S3, w, beta32, gamma, beta_u32, beta_u2_32) -> Tuple[int, int, Trace]:
    """One row of GpTermsK: all arguments are words (w = omega^i in gnark's radix)."""
    t = Trace(F, "GpTermsK")
    ln = "const U l = U::add_n(ld(L, i), gm), r = ..., o = ...   // < 2"
    gm = t.operand("gamma", gamma, 1, ln)
    l, r, o = (t.stated(nm, t.add_n(t.operand(nm.upper(), x, 1, ln), gm), 2, ln) for nm, x in (("l", L), ("r", R), ("o", O)))
    b, bu, bu2 = (t.operand(nm, x, 1, "beta, beta_u, beta_u2 arrive as 32 x") for nm, x in (("beta", beta32), ("beta_u", beta_u32), ("beta_u2", beta_u2_32)))
    wv = t.operand("omega^i", w, 1, "Fr wf = i < n / 2 ? tw[i] : Fr::neg(tw[i - n / 2])")
    out = []
    for name, cs in (("nu", ((l, b, wv), (r, bu, wv), (o, bu2, wv))),
                     ("de", ((l, b, t.operand("S1", S1, 1, "ld(S1, i)")), (r, b, t.operand("S2", S2, 1, "ld(S2, i)")), (o, b, t.operand("S3", S3, 1, "ld(S3, i)"))))):
        line = "U %s = U::mul_nr(U::add_n(l, ...), U::add_n(r, ...))   // factors < 4" % name
        fs = [t.stated("%s.factor%d" % (name, j), t.add_n(x, t.mul_nr(c, y, line)), 4, line) for j, (x, c, y) in enumerate(cs)]
        acc = t.stated(name + ".pair", t.mul_nr(fs[0], fs[1], line), 2, "Sums below 4 r, products below 2 r")
        acc = t.stated(name, t.mul_nr(acc, fs[2], line), 2, "Sums below 4 r, products below 2 r")
        out.append(t.canon1(acc, "U::template canon<1>(%s).pack(...)" % name))
    return out[0], out[1], t


def lazy_quotient(F: PolyField, p: dict) -> Tuple[int, Trace]:
    """One point of QuotientK.  `p` holds the point's WORDS under QuotientArgs' names (l r o z zs qk ql qr qm qo s1 s2 s3 x l0,
    qcp / pi2 / inj_tab / inj_delta as lists, the constants, zh_inv = the one the point uses)."""
    t = Trace(F, "QuotientK")
    ld = "const U l = ld(a.l, jj), r = ld(a.r, jj), o = ld(a.o, jj), z = ld(a.z, jj)   // SEMI-CANONICAL: below 2 r"
    l, r, o, z = (t.operand(k, p[k], 2, ld) for k in ("l", "r", "o", "z"))
    zs = t.operand("zs", p["zs"], 2, "const U zs = ld(zsp, is)")
    g1 = "U gate = U::add_n(U::mul_nr(ld(a.ql, i), l), U::mul_nr(ld(a.qr, i), r))   // 2 x (1 x 2: < 1.04)"
    a = t.stated("ql*l", t.mul_nr(t.operand("ql", p["ql"], 1, g1), l, g1), "1.04", g1)
    b = t.stated("qr*r", t.mul_nr(t.operand("qr", p["qr"], 1, g1), r, g1), "1.04", g1)
    gate = t.add_n(a, b)
    g2 = "gate = U::add_n(gate, U::mul_nr(ld(a.qm, i), U::mul_nr(l, r)))   // l r: 2 x 2, < 1.07; times qm < 1.02"
    lr = t.stated("l*r", t.mul_nr(l, r, g2), "1.07", g2)
    gate = t.add_n(gate, t.stated("qm*l*r", t.mul_nr(t.operand("qm", p["qm"], 1, g2), lr, g2), "1.02", g2))
    g3 = "gate = U::add_n(gate, U::mul_nr(ld(a.qo, i), o))   // < 1.04"
    gate = t.add_n(gate, t.stated("qo*o", t.mul_nr(t.operand("qo", p["qo"], 1, g3), o, g3), "1.04", g3))
    g4 = "gate = U::add_n(gate, ld(a.qk, i))   // < 1 (< 2 if ever semi-canonical): gate < 6.2"
    gate = t.stated("gate.trace", t.add_n(gate, t.operand("qk", p["qk"], 1, g4)), "6.2", g4)
    g5 = "// + 2 commitments (1 x 2: < 1.04 each) + 6 injections (1 x 1: < 1.02 each): gate < 14.4"
    for k in range(len(p["qcp"])):
        gate = t.add_n(gate, t.stated("qcp%d*pi2" % k, t.mul_nr(t.operand("qcp", p["qcp"][k], 1, g5), t.operand("pi2", p["pi2"][k], 2, g5), g5), "1.04", g5))
    for j in range(len(p["inj_tab"])):
        gate = t.add_n(gate, t.stated("inj%d" % j, t.mul_nr(t.operand("inj_delta", p["inj_delta"][j], 1, g5), t.operand("inj_tab", p["inj_tab"][j], 1, g5), g5), "1.02", g5))
    # the comment's total is for the full complement, whatever this launch carries
    gate = t.stated("gate", gate, "14.4", g5)
    s0 = "const U lg = U::add_n(l, gm), rg = U::add_n(r, gm), og = U::add_n(o, gm)   // < 3"
    gm = t.operand("gamma", p["gamma"], 1, s0)
    beta = t.operand("beta", p["beta"], 1, "const U gm = cst(a.gamma), beta = cst(a.beta)")
    lg, rg, og = (t.stated(nm, t.add_n(v, gm), 3, s0) for nm, v in (("lg", l), ("rg", r), ("og", o)))
    x = t.operand("x", p["x"], 1, "const U x = ld(a.x, i)")
    s1 = "U pa = U::mul_nr(zs, U::add_n(lg, U::mul_nr(beta, ld(a.s1, i))))   // factors < 3 + 1.02 < 4.1; products 2 x 4.1: < 1.13, then 1.13 x 4.1: < 1.08"
    prods = {}
    for name, first, cs in (("pa", zs, ((lg, beta, t.operand("s1", p["s1"], 1, s1)), (rg, beta, t.operand("s2", p["s2"], 1, s1)), (og, beta, t.operand("s3", p["s3"], 1, s1)))),
                            ("pb", z, ((lg, beta, x), (rg, t.operand("beta_u", p["beta_u"], 1, "U::mul_nr(cst(a.beta_u), x)"), x),
                                       (og, t.operand("beta_u2", p["beta_u2"], 1, "U::mul_nr(cst(a.beta_u2), x)"), x)))):
        acc = first
        for j, (v, c, y) in enumerate(cs):
            f = t.stated("%s.factor%d" % (name, j), t.add_n(v, t.stated("%s.bs%d" % (name, j), t.mul_nr(c, y, s1), "1.02", s1)), "4.1", s1)
            acc = t.stated("%s.%d" % (name, j), t.mul_nr(acc, f, s1), "1.13" if j == 0 else "1.08", s1)
        prods[name] = acc
    s2 = "const U perm = U::mul_nr(cst(a.alpha), U::template sub_k<2>(pa, pb))   // pb < 2; difference < 3.2; perm < 1.05"
    pb = t.stated("pb", prods["pb"], 2, s2)
    diff = t.stated("pa-pb", t.sub_k(2, prods["pa"], pb, s2), "3.2", s2)
    perm = t.stated("perm", t.mul_nr(t.operand("alpha", p["alpha"], 1, s2), diff, s2), "1.05", s2)
    s3 = "const U loc = U::mul_nr(cst(a.alpha2), U::mul_nr(ld(a.l0, i), U::template sub_k<1>(z, one)))   // z - 1 + r < 3; loc < 1.02"
    zm1 = t.stated("z-1", t.sub_k(1, z, t.operand("one", F.gnark.enc(1), 1, s3), s3), 3, s3)
    loc = t.stated("loc", t.mul_nr(t.operand("alpha2", p["alpha2"], 1, s3), t.mul_nr(t.operand("l0", p["l0"], 1, s3), zm1, s3), s3), "1.02", s3)
    s4 = "const U num = U::add_n(U::add_n(gate, perm), loc)   // < 14.4 + 1.05 + 1.02 < 17; times zh_inv: < 1.27"
    num = t.stated("num", t.add_n(t.add_n(gate, perm), loc), 17, s4)
    res = t.stated("res", t.mul_nr(t.operand("zh_inv", p["zh_inv"], 1, s4), num, s4), "1.27", s4)
    return t.canon1(res, "const U res = U::template canon<1>(U::mul_nr(cst(a.zh_inv[i & 3]), num))"), t


def lazy_merge(F: PolyField, parts: Sequence[int], rho_inv: Sequence[int], post: Sequence[int], G: int) -> Tuple[List[int], Trace]:
    """One column c' of subcoset_merge_kernel: parts[k] = part[k][c'], post[t] = post[c' + m t]; returns the G outputs."""
    t = Trace(F, "subcoset_merge_kernel")
    ln = "acc = U::add_n(acc, e ? U::mul_nr(U::unpack(a.rho_inv[e].l), v[k]) : v[k])   // sums of 8 products below 2 r each"
    v = [t.operand("part", w, 1, ln) for w in parts]
    out = []
    for tt in range(G):
        acc = v[0]
        for k in range(1, G):
            e = (k * tt) % G
            acc = t.add_n(acc, t.stated("term", t.mul_nr(t.operand("rho_inv", rho_inv[e], 1, ln), v[k], ln), 2, ln) if e else v[k])
        acc = t.stated("acc", acc, 16, ln)
        l2 = "const U res = U::template canon<1>(U::mul_nr(U::unpack(pw.l), acc))"
        out.append(t.canon1(t.stated("res", t.mul_nr(t.operand("post", post[tt], 1, l2), acc, l2), 2, l2), l2))
    return out, t


def lazy_eval_lane(F: PolyField, f: Sequence[int], pw: Sequence[int]) -> Tuple[int, Trace]:
    """One lane of EvalPartialK: up to 8 products, reduce_2p<8>, canon<1>"""
    t = Trace(F, "EvalPartialK")
    ln = "accu = U::add_n(accu, U::mul_nr(U::unpack(a0.l), U::unpack(b0.l)))   // 8 products below 2 r each"
    assert len(f) <= 8
    acc = LV(0, Fraction(0))
    for a, b in zip(f, pw):
        acc = t.add_n(acc, t.stated("f*pw", t.mul_nr(t.operand("f", a, 1, ln), t.operand("pw", b, 1, ln), ln), 2, ln))
    acc = t.stated("accu", acc, 16, ln)
    l2 = "U::template canon<1>(U::template reduce_2p<8>(accu)).pack(acc.l)"
    return t.canon1(t.reduce_2p(8, acc, l2), l2), t


def lazy_lincomb(F: PolyField, coef32: Sequence[int], vals: Sequence[int]) -> Tuple[int, Trace]:
    """One element of LincombK: up to LC_MAX products, reduce_2p<32>, canon<1>"""
    t = Trace(F, "LincombK")
    ln = "acc = U::add_n(acc, U::mul_nr(U::unpack(a.coef[k].l), U::unpack(v.l)))   // every product is below 2 r, up to LC_MAX of them add up below 64 r"
    assert len(vals) <= LC_MAX
    acc = LV(0, Fraction(0))
    for c, v in zip(coef32, vals):
        acc = t.add_n(acc, t.stated("c*f", t.mul_nr(t.operand("coef", c, 1, ln), t.operand("f", v, 1, ln), ln), 2, ln))
    acc = t.stated("acc", acc, 64, ln)
    l2 = "const U res = U::template canon<1>(U::template reduce_2p<32>(acc))"
    return t.canon1(t.reduce_2p(32, acc, l2), l2), t


def lazy_derive(F: PolyField, w: int, v: int) -> Tuple[int, Trace]:
    """One element of DerivePowersK before the sign: canon<1>(mul_nr(twu, in))"""
    t = Trace(F, "DerivePowersK")
    ln = "U r = U::template canon<1>(U::mul_nr(U::unpack(w.l), U::unpack(v.l)))"
    return t.canon1(t.stated("w*v", t.mul_nr(t.operand("twu", w, 1, ln), t.operand("in", v, 1, ln), ln), 2, ln), ln), t
