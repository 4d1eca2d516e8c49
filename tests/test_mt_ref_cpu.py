"""multiple_testing_method without a device: the NumPy restatement tests/mt_ref.py against hand-worked rationals, its order
relations, tie and NaN rules, the count-form tables against the sorted restatement, the per-entry functions of
safepy_amd/csrc/fdr_plan.h run through a stand-alone host program, backend.by_constant against mpmath, and the setting's
plumbing (validate_config, INI key, pickling, refusals, symbols)."""
import ctypes
import math
import os
import pickle
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fdr_cases as fc
import mt_ref as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')


# ------------------------------------------------------------------------------------------------------- by hand ----

HAND = (0.01, 0.04, 0.03, 0.005, 0.5)
HAND_EXACT = [Fraction(1, 100), Fraction(4, 100), Fraction(3, 100), Fraction(5, 1000), Fraction(1, 2)]
C5 = Fraction(137, 60)                                # 1 + 1/2 + 1/3 + 1/4 + 1/5
HAND_WANT = {
    # sorted .005 .01 .03 .04 .5; BH raw .025 .025 .05 .05 .5
    'fdr_bh': [Fraction(25, 1000), Fraction(5, 100), Fraction(5, 100), Fraction(25, 1000), Fraction(1, 2)],
    # the products (5 4 3 2 1) ps = .025 .04 .09 .08 .5: minimum from the right .025 .04 .08 .08 .5, maximum from the left
    # .025 .04 .09 .09 .5
    'hochberg': [Fraction(4, 100), Fraction(8, 100), Fraction(8, 100), Fraction(25, 1000), Fraction(1, 2)],
    'holm': [Fraction(4, 100), Fraction(9, 100), Fraction(9, 100), Fraction(25, 1000), Fraction(1, 2)],
    'bonferroni': [Fraction(5, 100), Fraction(2, 10), Fraction(15, 100), Fraction(25, 1000), Fraction(1)],
}
HAND_WANT['fdr_by'] = [min(v * C5, Fraction(1)) for v in HAND_WANT['fdr_bh']]


@pytest.mark.parametrize('method', mt.METHODS)
def test_hand_worked_family(method):
    """The restatement rounds a few times where the rationals do not: within 4 ulp of the rational rounded to f64, and exactly
    equal where every operation is exact in binary or a single rounding of the same quotient."""
    got = mt.family(HAND, method)
    want = np.array([float(v) for v in HAND_WANT[method]])
    assert abs(mt.by_verbatim(5) - float(C5)) <= 2 * np.spacing(float(C5))
    assert np.all(np.abs(got - want) <= 4 * np.spacing(want)), (method, got, want)
    # the same family as exact rationals through the same procedure, in exact arithmetic
    order = sorted(range(5), key=lambda i: HAND_EXACT[i])
    ps = [HAND_EXACT[i] for i in order]
    if method == 'bonferroni':
        adj = [min(v * 5, Fraction(1)) for v in ps]
    else:
        raw = {'fdr_bh': [v / Fraction(k, 5) for k, v in enumerate(ps, 1)],
               'fdr_by': [v / (Fraction(k, 5) / C5) for k, v in enumerate(ps, 1)]}.get(method, [v * (5 - k + 1) for k, v in enumerate(ps, 1)])
        if method == 'holm':
            adj = [max(raw[:k + 1]) for k in range(5)]
        else:
            adj = [min(raw[k:]) for k in range(5)]
        adj = [min(v, Fraction(1)) for v in adj]
    exact = [None] * 5
    for k, i in enumerate(order):
        exact[i] = adj[k]
    assert exact == HAND_WANT[method]


# ----------------------------------------------------------------------------------------------- order relations ----

def designed_families():
    for m in (1, 2, 5, 255, 1023, 1025):
        for method in ('fdr_bh', 'holm', 'hochberg'):
            names, p = mt.matrix(method, m)
            yield m, names, p


def test_order_relations_hold_on_the_bits():
    """bonferroni >= holm >= hochberg and fdr_by >= fdr_bh, exactly, on every designed family: monotone rounding of the same
    products and quotients.  (hochberg >= fdr_bh is NOT asserted: it fails by an ulp at k = 1 and k = count.)"""
    cells = differ = 0
    for m, names, p in designed_families():
        adj = {method: mt.rows(p, method) for method in mt.METHODS}
        ok = ~np.isnan(adj['fdr_bh'])                                 # rows without a NaN
        with np.errstate(invalid='ignore'):
            assert (adj['bonferroni'][ok] >= adj['holm'][ok]).all(), m
            assert (adj['holm'][ok] >= adj['hochberg'][ok]).all(), m
            assert (adj['fdr_by'][ok] >= adj['fdr_bh'][ok]).all(), m
        if m >= 255:
            small = [i for i, name in enumerate(names) if name == 'small']
            cells += adj['holm'][small].size
            differ += (adj['holm'][small] != adj['hochberg'][small]).sum()
    assert differ > cells // 2, (differ, cells)                       # the two scan directions are told apart


@pytest.mark.parametrize('method', mt.METHODS)
def test_shuffling_tie_groups_changes_nothing(method):
    rng = np.random.default_rng(3)
    base = np.repeat(rng.uniform(0.0, 0.02, size=40), rng.integers(1, 9, size=40))
    want = None
    for trial in range(4):
        perm = rng.permutation(base.size)
        got = np.empty(base.size)
        got[perm] = mt.family(base[perm], method)
        if want is None:
            want = got
        assert mt.same_bits(got, want), (method, trial)
    for value in np.unique(base):                                     # a tie group has one value
        assert np.unique(fc.bits(want[base == value])).size == 1


# ------------------------------------------------------------------------------------------- the count-form tables ----

@pytest.mark.parametrize('method', ('fdr_bh', 'fdr_by', 'holm', 'hochberg'))
@pytest.mark.parametrize('P', (1, 2, 10, 1000, 5119))
def test_count_form_tables_equal_the_sorted_restatement(method, P):
    """First position for Holm, last position for the others: the table of a histogram gives the sorted restatement's bits on
    count-ratio families with ties, NaN of both signs and -0.0."""
    for m in (1, 7, 257, 1031):
        names, p = fc.count_matrix(P, m, 0)
        want = mt.rows(p, method)
        got = np.stack([mt.counts_family(row, P, method) for row in p])
        assert not mt.differing(names, got, want), (method, P, m, mt.differing(names, got, want))
    p = fc.count_matrix(P, 257, 1)[1]
    for scope in ('neighborhoods', 'all'):
        want = mt.adjust(p, scope, method)
        if scope == 'all':
            got = mt.counts_family(p, P, method)
        else:
            got = np.stack([mt.counts_family(col, P, method) for col in p.T], axis=1)
        assert mt.same_bits(got, want), (method, P, scope)


# --------------------------------------------------------------------------------------------------- NaN and -0.0 ----

@pytest.mark.parametrize('method', mt.METHODS)
def test_nan_and_negative_zero_rules(method):
    rng = np.random.default_rng(5)
    base = rng.uniform(1e-4, 0.05, size=11)
    for pattern in (0x7FF8000000000000, fc.SIGN_NAN_BITS, fc.ALL_ONES_BITS, 0x7FF0000000000001):
        for at in (0, 5, 10):
            p = mt.with_bits(base, at, pattern)
            got = mt.family(p, method)
            if method in mt.POISONED:
                assert (fc.bits(got) == mt.QNAN_BITS).all()
            else:
                assert fc.bits(got)[at] == mt.QNAN_BITS and not np.isnan(np.delete(got, at)).any()
                # the numbers are members of a family of 11, the NaN counted: position k among the numbers, count 11
                ps = np.sort(np.delete(p, at))
                if method == 'bonferroni':
                    want = np.minimum(ps * 11.0, 1.0)
                else:
                    want = np.minimum(np.maximum.accumulate(ps * np.arange(11, 1, -1)), 1.0)
                assert mt.same_bits(np.sort(np.delete(got, at)), want)
    zeros = base.copy()
    zeros[3], zeros[7] = -0.0, 0.0
    plus = zeros.copy()
    plus[3] = 0.0
    got = mt.family(zeros, method)
    assert mt.same_bits(got, mt.family(plus, method))
    assert fc.bits(got)[3] == 0 and fc.bits(got)[7] == 0               # +0.0 on the bits
    assert mt.same_bits(mt.family([1.0], method), np.array([1.0])) and mt.same_bits(mt.family([np.inf], method), np.array([1.0]))


# ----------------------------------------------------------------------------------- fdr_plan.h, per-entry functions ----

# one line per command, doubles travel as their bits (hex) and come back as their bits (decimal)
#   step p rank count       -> fdr_step_raw
#   by p rank count c       -> fdr_by_raw
#   bonf p count            -> fdr_bonferroni_raw
#   raw proc p rank count c -> fdr_proc_raw
#   rule proc               -> fdr_proc_from_left fdr_proc_nan_poisons fdr_proc_sorts
#   enum                    -> the five FdrProcedure values and FDR_PROC_COUNT
DRIVER = r'''
#include <cstdio>
#include <cstring>
#include "fdr_plan.h"
static double d(unsigned long long b) { double v; std::memcpy(&v, &b, sizeof v); return v; }
static unsigned long long u(double v) { unsigned long long b; std::memcpy(&b, &v, sizeof b); return b; }
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char what[16];
    unsigned long long a, b, c, e;
    int proc;
    while (std::fscanf(f, "%15s", what) == 1) {
        if (!std::strcmp(what, "step")) {
            if (std::fscanf(f, "%llx %llx %llx", &a, &b, &c) != 3) return 3;
            std::printf("%llu\n", u(fdr_step_raw(d(a), d(b), d(c))));
        } else if (!std::strcmp(what, "by")) {
            if (std::fscanf(f, "%llx %llx %llx %llx", &a, &b, &c, &e) != 4) return 3;
            std::printf("%llu\n", u(fdr_by_raw(d(a), d(b), d(c), d(e))));
        } else if (!std::strcmp(what, "bonf")) {
            if (std::fscanf(f, "%llx %llx", &a, &b) != 2) return 3;
            std::printf("%llu\n", u(fdr_bonferroni_raw(d(a), d(b))));
        } else if (!std::strcmp(what, "raw")) {
            if (std::fscanf(f, "%d %llx %llx %llx %llx", &proc, &a, &b, &c, &e) != 5) return 3;
            std::printf("%llu\n", u(fdr_proc_raw(proc, d(a), d(b), d(c), d(e))));
        } else if (!std::strcmp(what, "rule")) {
            if (std::fscanf(f, "%d", &proc) != 1) return 3;
            std::printf("%d %d %d\n", fdr_proc_from_left(proc) ? 1 : 0, fdr_proc_nan_poisons(proc) ? 1 : 0, fdr_proc_sorts(proc) ? 1 : 0);
        } else if (!std::strcmp(what, "enum")) {
            std::printf("%d %d %d %d %d %d\n", FDR_PROC_BH, FDR_PROC_BY, FDR_PROC_HOLM, FDR_PROC_HOCHBERG, FDR_PROC_BONFERRONI, FDR_PROC_COUNT);
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    """run(lines) -> uint64 [len(lines), ...]: the header built for the host as a program of its own, with the address and
    undefined-behaviour sanitizers where the compiler links them (as tests/fdr_plan_driver.py does); nothing is loaded into Python."""
    d = tmp_path_factory.mktemp('mt_plan')
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed to build the planning header for the CPU'
    (d / 'drv.cpp').write_text(DRIVER)
    # -ffp-contract=off as the library's Makefile: every operation rounds
    base = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-ffp-contract=off', '-I' + CSRC, str(d / 'drv.cpp'), '-o', str(d / 'drv')]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    (d / 'in.txt').write_text('')
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0 or \
            subprocess.run([str(d / 'drv'), str(d / 'in.txt')], capture_output=True, env=env).returncode != 0:
        subprocess.run(base, check=True)

    def run(lines):
        lines = list(lines)
        (d / 'in.txt').write_text('\n'.join(lines) + '\n')
        out = subprocess.run([str(d / 'drv'), str(d / 'in.txt')], check=True, capture_output=True, text=True, env=env).stdout
        rows = [[int(x) for x in ln.split()] for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return np.array(rows, dtype=np.uint64)
    return run


def hx(v):
    return '%x' % int(np.float64(v).view(np.uint64))


def test_plan_header_per_entry_functions(plan):
    """The new FDR_HD functions on designed operands -- subnormals, the zero, 1, values that round, +inf, NaN; ranks 1, the
    middle and count; counts 1, 3, 4373, 2^31 - 1, 2 10^8 -- against the NumPy operations, bit for bit; the enum numbers the
    procedures as safe_hip.h does, and the scan direction / NaN rule / sort need of each."""
    assert plan(['enum'])[0].tolist() == [0, 1, 2, 3, 4, 5]
    rules = plan('rule %d' % k for k in range(5))
    assert rules.tolist() == [[0, 1, 1], [0, 1, 1], [1, 0, 1], [0, 1, 1], [0, 0, 0]]
    values = [0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 0.001, 1 / 3.0, 0.05, 0.1, 0.7, np.nextafter(1.0, 0.0), 1.0, 3.0, np.inf, np.nan]
    lines, want = [], []
    for count in (1, 3, 4373, 2 ** 31 - 1, 200000000):
        c_by = mt.by_verbatim(min(count, 1 << 20)) + (count > (1 << 20))
        for rank in sorted({1, (count + 1) // 2, count}):
            for p in values:
                p, r, n, c = np.float64(p), np.float64(rank), np.float64(count), np.float64(c_by)
                with np.errstate(all='ignore'):
                    cases = [('step %s %s %s' % (hx(p), hx(r), hx(n)), np.float64(np.int64(count) - np.int64(rank) + 1) * p),
                             ('by %s %s %s %s' % (hx(p), hx(r), hx(n), hx(c)), p / ((r / n) / c)),
                             ('bonf %s %s' % (hx(p), hx(n)), p * n),
                             ('raw 0 %s %s %s %s' % (hx(p), hx(r), hx(n), hx(c)), p / (r / n)),
                             ('raw 1 %s %s %s %s' % (hx(p), hx(r), hx(n), hx(c)), p / ((r / n) / c)),
                             ('raw 2 %s %s %s %s' % (hx(p), hx(r), hx(n), hx(c)), np.float64(count - rank + 1) * p),
                             ('raw 3 %s %s %s %s' % (hx(p), hx(r), hx(n), hx(c)), np.float64(count - rank + 1) * p)]
                for line, w in cases:
                    lines.append(line)
                    want.append(np.float64(w))
    got = plan(lines)[:, 0].view(np.float64)
    want = np.array(want)
    bad = [lines[i] for i in range(len(lines)) if not (np.isnan(want[i]) and np.isnan(got[i])) and fc.bits(got[i:i + 1])[0] != fc.bits(want[i:i + 1])[0]]
    assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------------- by_constant ----

def test_by_constant():
    """The verbatim expression up to 2^24 terms; beyond that chunks joined with math.fsum, checked against mpmath.harmonic: no
    worse, in units of 2^-53 H, than the verbatim expression itself is at 2^24, times 2 for the join."""
    mpmath = pytest.importorskip('mpmath')
    from safepy_amd import backend as be
    for count in (1, 2, 5, 1000, 4373, 3971 * 1000, 1 << 24):
        assert be.by_constant(count) == mt.by_verbatim(count), count
    assert be.by_constant(5) == be.by_constant(5) and 5 in be._by_constants                 # cached per count
    with pytest.raises(ValueError):
        be.by_constant(0)
    mpmath.mp.prec = 200

    def units(value, count):
        h = mpmath.harmonic(count)
        return float(abs(mpmath.mpf(value) - h) / (h * mpmath.mpf(2) ** -53))

    at_limit = units(mt.by_verbatim(1 << 24), 1 << 24)
    print('by_constant: the verbatim expression at 2^24 is %.2f units of 2^-53 H from mpmath.harmonic' % at_limit)
    bound = 2 * max(at_limit, 1.0)                    # (a verbatim sum that happened to round exactly still allows one unit per part)
    for count in ((1 << 24) + 1, 3 * (1 << 24) + 5):
        got = units(be.by_constant(count), count)
        print('by_constant(%d) = %r: %.2f units (bound %.2f)' % (count, be.by_constant(count), got, bound))
        assert got <= bound, (count, got, bound)


# ------------------------------------------------------------------------------------------ settings and plumbing ----

def test_settings_ini_and_pickle(tmp_path):
    import safepy_amd
    from safepy_amd import backend as be
    from safepy_amd import safe
    assert tuple(be.MT_METHODS) == mt.METHODS == safe._MT_METHODS and be.MT_METHODS == mt.NUMBERS
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.multiple_testing_method == 'fdr_bh'
    for bad in ('bh', 'BH', 'sidak', 'holm-sidak', 'fdr_BY', '', 0, None, ['holm']):
        sf.multiple_testing_method = bad
        with pytest.raises(ValueError, match='multiple_testing_method') as err:
            sf.validate_config()
        assert 'fdr_bh, fdr_by, holm, hochberg, bonferroni' in str(err.value)
        assert sf.multiple_testing_method == 'fdr_bh'                         # restored
    for good in mt.METHODS:
        sf.multiple_testing_method = good
        sf.validate_config()

    ini = tmp_path / 'mt.ini'
    ini.write_text('[Analysis parameters]\nmultipleTestingMethod = holm\n')
    assert safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False).multiple_testing_method == 'holm'
    ini.write_text('[Analysis parameters]\nmultipleTestingMethod =\n')
    assert safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False).multiple_testing_method == 'fdr_bh'
    ini.write_text('[Analysis parameters]\nmultipleTestingMethod = sidak\n')
    with pytest.raises(ValueError, match='multiple_testing_method'):
        safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)

    sf.multiple_testing_method = 'hochberg'
    assert pickle.loads(pickle.dumps(sf)).multiple_testing_method == 'hochberg'
    state = sf.__getstate__()
    del state['multiple_testing_method']                                      # an object pickled before the setting existed
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.multiple_testing_method == 'fdr_bh'
    old.validate_config()


def test_refusals_before_any_device_work():
    """A bad method, and everything that refuses multiple_testing without a device, under every method: the results stay."""
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.node2attribute = np.zeros((5, 2))
    marks = {name: object() for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')}
    for name, mark in marks.items():
        setattr(sf, name, mark)
    cases = [(dict(how='randomization', multiple_testing=True, multiple_testing_method='sidak'), 'multiple_testing_method'),
             (dict(how='hypergeometric', multiple_testing=True, multiple_testing_method=3), 'multiple_testing_method')]
    cases += [(dict(how='randomization', familywise_adjustment='maxT', multiple_testing=True, multiple_testing_method=method), 'multiple_testing')
              for method in mt.METHODS]
    for kwargs, message in cases:
        with pytest.raises(ValueError, match=message):
            sf.compute_pvalues(**kwargs)
        for name, mark in marks.items():
            assert getattr(sf, name) is mark, (kwargs, name)
        sf.familywise_adjustment, sf.multiple_testing, sf.enrichment_type, sf.multiple_testing_method = 'none', False, 'auto', 'fdr_bh'


def test_symbols_are_declared_bound_and_exported():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    assert re.search(r'#define SAFE_HIP_ABI_VERSION 9\b', header)             # additive: the version stays
    for name, number in (('FDR_BH', 0), ('FDR_BY', 1), ('HOLM', 2), ('HOCHBERG', 3), ('BONFERRONI', 4)):
        assert re.search(r'#define SAFE_MT_%s %d\b' % (name, number), header), name
        assert getattr(_lib, 'MT_' + name) == number
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (('safe_mt_adjust_scope', 14), ('safe_mt_adjust_matrix', 8)):
        found = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, code)
        assert found and len(found.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert hasattr(raw, name)
    for name in ('MT_METHODS', 'by_constant', 'mt_adjust_scope', 'mt_adjust_matrix'):
        assert hasattr(backend, name), name
    # refused before a device is touched: NULL arguments, a method outside 0 ... 4, a constant that is no harmonic sum
    one = ctypes.c_void_p(8)
    assert _lib.lib.safe_mt_adjust_matrix(None, 1, 1, 0, 0, 0.0, 0, None) == _lib.E_VALUE
    assert b'NULL argument' in _lib.lib.safe_last_error()
    assert _lib.lib.safe_mt_adjust_scope(None, 1, 1, 0, 0, 0.05, 0, 0, 0.0, None, None, None, None, None) == _lib.E_VALUE
    for method in (-1, 5):
        assert _lib.lib.safe_mt_adjust_matrix(one, 1, 1, 0, method, 1.0, 0, one) == _lib.E_VALUE
        assert b'bad method' in _lib.lib.safe_last_error()
    for c in (0.0, 0.999, -2.0, math.inf, math.nan):
        assert _lib.lib.safe_mt_adjust_matrix(one, 1, 1, 0, 1, c, 0, one) == _lib.E_VALUE
        assert b'by_constant' in _lib.lib.safe_last_error()


@pytest.mark.parametrize('method', mt.METHODS)
def test_restatement_against_statsmodels(method):
    multitest = pytest.importorskip('statsmodels.stats.multitest')
    name = {'hochberg': 'simes-hochberg'}.get(method, method)
    for m in (1, 2, 5, 257, 1025):
        for rname, row in mt.designed_rows(method, m):
            if np.isnan(row).any() or (row < 0).any() or np.signbit(row).any():
                continue
            want = multitest.multipletests(row, method=name)[1]
            assert np.array_equal(mt.family(row, method), want), (method, m, rname)
