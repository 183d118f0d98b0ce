"""The LocalMapping / LoopClosing / initialiser matcher gates (match2_gate_cases): the oracle gives the hand-written answers, the kernel logic (emulator) gives them too
and equals the oracle everywhere."""
import pytest
import match2_gate_cases as g2


def test_case_contents(oracle):
    g2.check_case_contents(oracle)


@pytest.mark.parametrize('name', g2.NAMES)
def test_gate_case_emu(emu, oracle, name):
    c = g2.CASE[name]
    g2.check_kat(oracle, c)
    g2.run_case(emu, oracle, c, exact=True)


@pytest.mark.parametrize('ks,nlevels', [(range(9), 8), ((7, 8), 10)])
def test_level_boundary_sweep_emu(emu, oracle, ks, nlevels):
    """PredictScale through sgx_match_fuse_search_sim3 on 13 consecutive floats around every level boundary 1.2f^k; the oracle shows both outcomes around every boundary"""
    want = g2.sweep_fs3(oracle, ks, nlevels)
    for j, k in enumerate(ks): assert set(want[13 * j:13 * j + 13]) == {min(k, nlevels - 1), min(k + 1, nlevels - 1)}, (k, want[13 * j:13 * j + 13])
    assert g2.sweep_fs3(emu, ks, nlevels) == want


@pytest.mark.parametrize('nn', [257, 600])
def test_sizes_nodes_emu(emu, oracle, nn):
    g2.check_sizes_nodes(emu, oracle, nn)


@pytest.mark.parametrize('nm', [255, 256, 257])
def test_sizes_points_emu(emu, oracle, nm):
    g2.check_sizes_points(emu, oracle, nm)


@pytest.mark.parametrize('nk,nm', [(1025, 1025), (2049, 600), (600, 2049)])
def test_sizes_workgroup_emu(emu, oracle, nk, nm):
    g2.check_sizes_workgroup(emu, oracle, nk, nm)


def test_sizes_init_emu(emu, oracle):
    g2.check_sizes_init(emu, oracle)
