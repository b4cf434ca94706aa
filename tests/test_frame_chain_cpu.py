"""The lz4f block chain walk without a GPU (corpus and model: tests/chaingen.py).

1. On every case the oracle's decompress_frame and the two Python frame models agree, so any of them can state what the
   GPU calls must answer (tests/test_gpu_frame_chain.py).
2. The shared chain step of zig-lz4_amd/csrc/zlz4_frame_batch.hpp, compiled for the host with AddressSanitizer and
   UBSan into tests/chain_walk_check.cpp, walks every case as chaingen.walk does: header status, block count, cursor, ending.
3. The host block-count helper of the same header gives chaingen.walk's count on every case.
"""
import os
import shutil
import subprocess
import sys

import pytest

import chaingen as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_sizes as zs  # noqa: E402


def test_the_corpus():
    fr = g.frames()
    assert len(fr) == 16 and len({f for _, _, _, f in fr}) == 16
    cs = g.cases()
    assert len(cs) == sum(len(f) + 1 for _, _, _, f in fr) and 2000 < len(cs) < 2600
    ends = {g.walk(b)[3] for _, b in cs}
    assert ends == {g.BOUNDARY, g.WORD_CUT, g.END_MARK, g.DATA_CUT, g.CKS_CUT, g.NO_HEADER}
    for name, bc, cc, f in fr:
        hs, nb, pos, end = g.walk(f)
        if name.endswith("_huge_word"):
            assert (nb, pos, end) == (0, g.HEADER + 4, g.DATA_CUT)
        else:
            assert nb == (4 if name.endswith("_zero_stored") else 3) and end == g.END_MARK
            assert pos + (4 if cc else 0) + (8 if name.endswith("_trailing") else 0) == len(f)
            assert zs.frame_size(f) == g.CONTENT_SIZE, name


def test_oracle_and_models_agree_on_every_case(oracle):
    bad = []
    for name, b in g.cases():
        o = oracle.decompress_frame(b, 4096)
        o = o if isinstance(o, int) else len(o)
        s, l = zs.frame_size(b), lf.decompress_frame_linked(b, 4096)[0]
        if not (o == s == l):
            bad.append((name, o, s, l))
    assert not bad, (len(bad), bad[:8])


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    """tests/chain_walk_check.cpp over every case -> [(header status, blocks, cursor, ending, helper's count)]"""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc: the host build of the chain step was NOT checked")
    tmp = tmp_path_factory.mktemp("chain")
    exe, data = str(tmp / "chain_walk_check"), str(tmp / "cases.bin")
    cs = g.cases()
    with open(data, "wb") as f:
        f.write(len(cs).to_bytes(4, "little"))
        for _, b in cs:
            f.write(len(b).to_bytes(4, "little") + b)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "chain_walk_check.cpp")], cwd=str(tmp))
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout[-2000:] + out.stderr[-4000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == len(cs)
    return [(int(r[0]), int(r[1]), int(r[2]), r[3], int(r[4])) for r in rows]


def test_host_build_of_the_chain_step_walks_as_the_model(host_walk):
    bad = [(name, got[:4], g.walk(b)) for (name, b), got in zip(g.cases(), host_walk) if got[:4] != g.walk(b)]
    assert not bad, (len(bad), bad[:8])


def test_host_block_count_helper_gives_the_models_count(host_walk):
    bad = [(name, got[4], g.walk(b)[1]) for (name, b), got in zip(g.cases(), host_walk) if got[4] != g.walk(b)[1]]
    assert not bad, (len(bad), bad[:8])
