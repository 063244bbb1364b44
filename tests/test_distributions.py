"""The shared spec's samplers (include/rtw_scalar.h) against their closed-form distributions.

Kernel and oracle draw from the same header, so a square taken for a disc or a cube for a ball is invisible to
the parity tests.  tests/native/dist_check.c draws 2^26 values from each sampler (64 fixed streams: the figures
do not depend on the thread count) and prints raw f64 sums and 64-bin histograms; here every moment must sit
within 5 standard errors of its closed form and every histogram's chi^2 within 5 sqrt(2 dof) of its dof, the
standard errors from the closed-form variances.  About 3 s on 16 threads."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N = 1 << 26
BOUND = 5.0  # as tests/analytic_scenes.Z_BOUND: a choice of false-alarm rate (about 6e-7 a figure), not a measurement


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return str(max(1, min(n, 16)))


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dist") / "dist_check"
    subprocess.run(["gcc", "-O2", "-std=c11", "-march=x86-64-v3", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "dist_check.c"), "-lm", "-lpthread"], check=True)
    out = subprocess.run([str(exe), _threads()], capture_output=True, text=True, timeout=600, check=True)
    fig = {}
    for line in out.stdout.splitlines():
        key, *vals = line.split()
        fig[key] = np.array([float(v) for v in vals]) if key.endswith(".sums") else np.array([int(v) for v in vals])
    assert all(fig[k][0] == N for k in fig if k.endswith(".n"))
    return fig


def near(value: float, expect: float, variance: float, what: str) -> None:
    """|the mean of N draws - its expectation| <= 5 standard errors, from the closed-form single-draw variance."""
    sigma = np.sqrt(variance / N)
    assert abs(value - expect) <= BOUND * sigma, f"{what}: {value} vs {expect}, {(value - expect) / sigma:+.2f} sigma"


def fits(hist, probs, what: str) -> None:
    """Pearson's chi^2 of the counts against the bin probabilities, within 5 sqrt(2 dof) of dof."""
    hist, probs = np.asarray(hist, np.float64), np.asarray(probs, np.float64)
    assert hist.sum() == N and abs(probs.sum() - 1.0) < 1e-12
    chi2, dof = float(((hist - N * probs) ** 2 / (N * probs)).sum()), len(probs) - 1
    assert abs(chi2 - dof) <= BOUND * np.sqrt(2.0 * dof), f"{what}: chi2 {chi2:.1f} on {dof} dof"


FLAT = np.full(64, 1.0 / 64)


def moments(fig, name, mean, var, fourth_central):
    """The first two sums of `name` against a distribution's mean and variance."""
    s = fig[name + ".sums"]
    m = s[0] / N
    near(m, mean, var, name + " mean")
    near(s[1] / N - 2 * mean * m + mean * mean, var, fourth_central - var * var, name + " variance")


def test_gen_f32(figures):
    """Standard f32: on the 2^-24 grid, never 1, mean 1/2, variance 1/12, flat."""
    assert figures["gen_f32.counts"][0] == 0 and figures["gen_f32.counts"][1] == 0
    moments(figures, "gen_f32", 0.5, 1 / 12, 1 / 80)
    fits(figures["gen_f32.hist0"], FLAT, "gen_f32")


def test_uniform_and_gen_range(figures):
    """Uniform::new(0, 1/47).sample and gen_range(-1..3): inside [low, high), flat, the moments of U(low, high)."""
    high = float(np.float32(1.0) / np.float32(47.0))
    assert figures["uniform.counts"][0] == 0 and figures["range.counts"][0] == 0
    moments(figures, "uniform", high / 2, high**2 / 12, high**4 / 80)
    moments(figures, "range", 1.0, 16 / 12, 256 / 80)
    fits(figures["uniform.hist0"], FLAT, "uniform")
    fits(figures["range.hist0"], FLAT, "gen_range")


def test_gen_range_never_reaches_high(figures):
    """[100, 101): scale * max + low rounds up to high there (the checker says so), so Uniform::new has to shrink
    its scale and gen_range has to redraw (U5); neither may ever return high."""
    c, s = figures["tight.counts"], figures["tight.sums"]
    assert c[0] == 1, "the range does not exercise the shrink loop"
    assert c[1] == 0 and c[2] == 0
    near(s[0] / N, 100.5, 1 / 12, "Uniform::new(100, 101) mean")
    near(s[1] / N, 100.5, 1 / 12, "gen_range(100..101) mean")


def test_gen_bool_half(figures):
    near(figures["bool.counts"][0] / N, 0.5, 0.25, "gen_bool(0.5)")


def test_gen_range_u32(figures):
    """gen_range(0..n) for n = 3, 7 and 2^31 + 1 (most draws rejected by the zone there): in range and uniform."""
    for name, n in (("u32_3", 3), ("u32_7", 7)):
        assert figures[name + ".counts"][0] == 0 and not figures[name + ".hist0"][n:].any()
        fits(figures[name + ".hist0"][:n], np.full(n, 1.0 / n), name)
    n = (1 << 31) + 1
    assert figures["u32_big.counts"][0] == 0
    edges = np.array([-(-(b * n) // 64) for b in range(65)], np.float64)  # the least v with v * 64 // n >= b
    fits(figures["u32_big.hist0"], np.diff(edges) / n, "u32_big")


def test_unit_disc(figures):
    """r^2 and the angle uniform (a square would fail both); E x = 0, E x^2 = 1/4, E xy = 0."""
    s = figures["disc.sums"]
    assert figures["disc.counts"][0] == 0
    near(s[0] / N, 0.0, 1 / 4, "disc x")
    near(s[1] / N, 0.0, 1 / 4, "disc y")
    near(s[2] / N, 1 / 4, 1 / 8 - 1 / 16, "disc x^2")
    near(s[3] / N, 1 / 4, 1 / 8 - 1 / 16, "disc y^2")
    near(s[4] / N, 0.0, 1 / 24, "disc xy")
    fits(figures["disc.hist0"], FLAT, "disc r^2")
    fits(figures["disc.hist1"], FLAT, "disc angle")


def test_unit_sphere(figures):
    """On the sphere; z (and x) uniform, Archimedes; E x_i = 0, E x_i x_j = delta_ij / 3."""
    s = figures["sphere.sums"]
    assert s[9] <= 2.0**-21
    for i in range(3):
        near(s[i] / N, 0.0, 1 / 3, f"sphere x{i}")
        near(s[3 + i] / N, 1 / 3, 1 / 5 - 1 / 9, f"sphere x{i}^2")
        near(s[6 + i] / N, 0.0, 1 / 15, "sphere " + ("xy", "xz", "yz")[i])
    fits(figures["sphere.hist0"], FLAT, "sphere z")
    fits(figures["sphere.hist1"], FLAT, "sphere x")


def test_unit_ball(figures):
    """Inside the ball; r^3 uniform (a cube, or a cylinder accepted on x^2 + y^2, fails it); z has the density
    (3/4)(1 - z^2)."""
    s = figures["ball.sums"]
    assert figures["ball.counts"][0] == 0
    for i in range(3):
        near(s[i] / N, 0.0, 1 / 5, f"ball x{i}")
    fits(figures["ball.hist0"], FLAT, "ball r^3")
    z = np.linspace(-1.0, 1.0, 65)
    fits(figures["ball.hist1"], np.diff(0.5 + 0.75 * (z - z**3 / 3)), "ball z")


@pytest.mark.parametrize("name", ["lobe_z", "lobe_tilted"])
def test_cosine_lobe(figures, name):
    """unit(n + unit_sphere): cos^2 of the angle to n uniform, so E cos = 2/3 with variance 1/2 - 4/9."""
    assert figures[name + ".counts"][0] == 0
    near(figures[name + ".sums"][0] / N, 2 / 3, 1 / 2 - 4 / 9, name + " cos")
    fits(figures[name + ".hist0"], FLAT, name + " cos^2")
