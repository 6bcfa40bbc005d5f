"""hg_frag_sketch_seq_dev (libhypergen_frag.so) on a 40.3 kbp sequence: the windows of 1 000 bases every 1 000 and every 500 are
sketched as offsets into the one resident buffer, where bases follow every window's end; each window's hypervector, norm and
hash count equal hg_sketch_batch_dev on that window copied out as a genome of its own, with other bytes behind it.  A window
whose k-mers ran on into the next window's bases would differ: the genome's end masks them, not the buffer's.  k = 21 and
k = 41; window 0 ends on a non-base byte, one window is all lower case, one holds a run of N."""
import numpy as np
import pytest
import torch

import frag_ref

pytestmark = pytest.mark.gpu

LEN, W, HV_D = 40_300, 1000, 1024
BASES = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_frag()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def sequence():
    rng = np.random.default_rng(403)
    seq = rng.choice(BASES, LEN)
    seq[0] = ord("N")                      # (hg_read_merge_seq starts every record with one)
    seq[W - 1] = ord("N")                  # window 0 ends on a non-base byte
    seq[3 * W:4 * W] |= 0x20               # a window in lower case
    seq[7 * W + 480:7 * W + 540] = ord("N")  # a run across the middle of a window and the start of an overlapping one
    d_seq = torch.from_numpy(np.concatenate((seq, rng.choice(BASES, 64)))).to("cuda:0")  # bases behind the end, too
    torch.cuda.synchronize()
    return seq, d_seq


def windows_alone(hg, ctx, seq, plan, params):
    """hg_sketch_batch_dev on the windows copied out: every window at a multiple of 64, 'T's behind it"""
    offs, total = [], 0
    for _, n in plan:
        offs.append(total)
        total += (n + 32 + 63) // 64 * 64
    host = np.full(total + 64, ord("T"), np.uint8)
    for (s, n), o in zip(plan, offs):
        host[o:o + n] = seq[s:s + n]
    m = len(plan)
    d = torch.from_numpy(host).to("cuda:0")
    hv = torch.zeros((m, HV_D), dtype=torch.int16, device="cuda:0")
    n2 = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    nh = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sketch_batch_dev(d.data_ptr(), offs, [n for _, n in plan], params, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
    ctx.sync()
    return hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("ksize", [21, 41])
@pytest.mark.parametrize("step", [1000, 500])
def test_every_window_equals_its_bytes_sketched_alone(hg, ctx, sequence, step, ksize):
    seq, d_seq = sequence
    params = hg.default_params(ksize=ksize, scaled=10, hv_d=HV_D)
    plan = frag_ref.plan(LEN, W, step)
    assert len(plan) == (40 if step == W else 80) and plan[-1] == ((39_000, 1000) if step == W else (39_500, 800))
    starts, lens, hv, n2, nh = ctx.frag_sketch_seq_dev(d_seq.data_ptr(), LEN, params, W, step)
    assert list(zip(starts.tolist(), lens.tolist())) == plan
    want_hv, want_n2, want_nh = windows_alone(hg, ctx, seq, plan, params)
    assert (nh == want_nh).all() and (n2 == want_n2).all() and (hv == want_hv).all()
    assert 40 < int(nh.min()) and int(nh.max()) < 200 and len({x.tobytes() for x in hv}) == len(plan)  # ~98 hashes each, all different


def test_short_and_empty_sequences_are_one_window(hg, ctx, sequence):
    seq, d_seq = sequence
    params = hg.default_params(ksize=21, scaled=10, hv_d=HV_D)
    for n in (0, 20, 999):
        starts, lens, hv, n2, nh = ctx.frag_sketch_seq_dev(d_seq.data_ptr(), n, params, W, W)
        assert (starts.tolist(), lens.tolist()) == ([0], [n])
        want_hv, want_n2, want_nh = windows_alone(hg, ctx, seq, [(0, n)], params)
        assert (nh == want_nh).all() and (n2 == want_n2).all() and (hv == want_hv).all() and (n >= 21 or nh[0] == 0)
    with pytest.raises(hg.HgError):
        ctx.frag_sketch_seq_dev(d_seq.data_ptr(), LEN, params, W, W + 4)
