"""The LocalMapping / LoopClosing / initialiser matcher gates (match2_gate_cases) on the device: the product library gives the hand-written answers and equals the oracle."""
import pytest
import match2_gate_cases as g2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', g2.NAMES)
def test_gate_case_gpu(gpulib, oracle, name):
    """new-map-point cases: flags equal to the oracle's, unprojected positions bit-equal, SVD positions within 2e-3 relative (the figure is printed)"""
    diff = g2.run_case(gpulib, oracle, g2.CASE[name], exact=False)
    if diff is not None: print('%s: largest position difference per branch %r' % (name, diff))


@pytest.mark.parametrize('ks,nlevels', [(range(9), 8), ((7, 8), 10)])
def test_level_boundary_sweep_gpu(gpulib, oracle, ks, nlevels):
    """the device's PredictScale in sgx_match_fuse_search_sim3 against glibc's ceilf(logf(ratio) / log_scale_factor) on 13 consecutive floats around every boundary 1.2f^k"""
    import match_gate_cases as mg
    got = g2.sweep_fs3(gpulib, ks, nlevels); want = g2.sweep_fs3(oracle, ks, nlevels)
    bad = [(k, float(r), g, w) for (k, r), g, w in zip(mg.sweep_ratios(ks), got, want) if g != w]
    print('fuse_search_sim3 sweep, nlevels %d: %d of %d ratios disagree' % (nlevels, len(bad), len(got)), bad)
    assert not bad


@pytest.mark.parametrize('nn', [257, 600])
def test_sizes_nodes_gpu(gpulib, oracle, nn):
    g2.check_sizes_nodes(gpulib, oracle, nn)


@pytest.mark.parametrize('nm', [255, 256, 257])
def test_sizes_points_gpu(gpulib, oracle, nm):
    g2.check_sizes_points(gpulib, oracle, nm)


@pytest.mark.parametrize('nk,nm', [(1025, 1025), (2049, 600), (600, 2049)])
def test_sizes_workgroup_gpu(gpulib, oracle, nk, nm):
    g2.check_sizes_workgroup(gpulib, oracle, nk, nm)


def test_sizes_init_gpu(gpulib, oracle):
    g2.check_sizes_init(gpulib, oracle)
