"""The shortest float-to-text routine of the device formatter (safepy_amd/csrc/fmt_f64.h, a __host__ __device__ header) built
for the host with the system C++ compiler, against NumPy's astype(str) -- what pandas' to_csv writes for float blocks -- and
CPython's repr(float) on random bit patterns and on the values where shortest-digit algorithms go wrong.  No GPU needed; the
device path is pinned by tests/test_gpu_output_files.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "fmt_f64.h"
int main(int argc, char **argv) {
    FILE *f = std::fopen(argv[1], "rb");
    std::vector<uint64_t> v;
    uint64_t b;
    while (std::fread(&b, 8, 1, f) == 1) v.push_back(b);
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    char buf[64];
    for (uint64_t x : v) {
        const int n = f64_text(x, buf);
        if (n != f64_text(x, nullptr) || n > F64_TEXT_MAX) return 3;
        buf[n] = '\n';
        std::fwrite(buf, 1, n + 1, o);
    }
    std::fclose(o);
    return 0;
}
'''


def curated():
    """The values of the issue's list: specials, powers of ten and two with their neighbours, the notation switches, integers
    around 2^53, the NES table -log10(k / P)."""
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
         9.999999999999999e-05, 1e-4, 9999999999999998.0, 1e16, 0.1, 0.3, 2.0 / 3.0, 123456.789]
    v += [float('1e%d' % k) for k in range(-323, 309)]
    v += [2.0 ** k for k in range(-1074, 1024)]
    v += [float(2 ** 53 + d) for d in range(-8, 9)]
    for p in (100, 1000, 10000):
        v += list(-np.log10(np.arange(1, p + 1) / p))
    bits = np.array(v, dtype=np.float64).view(np.uint64)
    with np.errstate(over='ignore'):
        bits = np.concatenate([bits, bits + np.uint64(1), bits - np.uint64(1)])
    x = bits.view(np.float64)
    return np.concatenate([x, -x])


@pytest.fixture(scope='module')
def formatter(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed to build the formatter for the CPU'
    d = tmp_path_factory.mktemp('fmt')
    subprocess.run([sys.executable, os.path.join(CSRC, 'gen_pow5.py'), str(d / 'pow5_table.h')], check=True)
    (d / 'drv.cpp').write_text(DRIVER)
    subprocess.run([cxx, '-O2', '-std=c++17', '-I' + CSRC, '-I' + str(d), str(d / 'drv.cpp'), '-o', str(d / 'drv')], check=True)

    def run(x):
        np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tofile(str(d / 'in.bin'))
        subprocess.run([str(d / 'drv'), str(d / 'in.bin'), str(d / 'out.txt')], check=True)
        return open(str(d / 'out.txt')).read().split('\n')[:-1]
    return run


def expect(x):
    return ['' if s == 'nan' else s for s in map(repr, x.tolist())]


def test_curated_values_equal_numpy(formatter):
    x = curated()
    want = ['' if s == 'nan' else s for s in x.astype(str).tolist()]
    assert want == expect(x)                       # NumPy and CPython agree on every one of them
    got = formatter(x)
    bad = [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:10]
    assert formatter(np.array([9.999999999999999e-05, 1e-4, 9999999999999998.0, 1e16, 5e-324, -0.0, -np.inf])) == \
        ['9.999999999999999e-05', '0.0001', '9999999999999998.0', '1e+16', '5e-324', '-0.0', '-inf']


def test_random_bit_patterns_equal_repr(formatter):
    rng = np.random.default_rng(2024)
    x = rng.integers(0, 2 ** 64, size=1_000_000, dtype=np.uint64, endpoint=False).view(np.float64)
    got, want = formatter(x), expect(x)
    bad = [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:10]
    sub = x[:50_000]
    assert ['' if s == 'nan' else s for s in sub.astype(str).tolist()] == got[:50_000]


def test_short_decimals_and_integers_equal_repr(formatter):
    """Values with few significant digits take the exact-tie branches that random bit patterns almost never reach."""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(-10 ** 17, 10 ** 17, 200_000).astype(np.float64), np.round(rng.uniform(-1e6, 1e6, 200_000), 3),
                        rng.integers(0, 10 ** 6, 200_000) / 10.0 ** rng.integers(0, 25, 200_000),
                        rng.integers(1, 10 ** 6, 200_000) * 10.0 ** rng.integers(-300, 300, 200_000), np.arange(-50_000, 50_000) * 0.5])
    got, want = formatter(x), expect(x)
    bad = [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:10]
