"""Two switches inside the host layer that pick a different launch sequence for the same call, each
pinned from both sides:

* nw_verify_certs uploads the preamble state with its inputs (no preamble kernels) up to 16,384 votes
  and runs the preamble kernels above; 16,385 votes is also the first size at which the signatures
  are grouped by signer.  Both sizes, with corrupted signatures, an empty certificate and unclaimed
  votes, against the CPU reference (nw_ref) on every certificate and against nw_verify_certs_dev.
* cached-key nw_verify_strict_many / nw_verify_batch take the one-DMA path while the staged input
  stays below 2 MiB and the segment-by-segment path from there; verdicts from the Python oracle.
"""
import numpy as np
import pytest

import ed25519_oracle as o
import nw_ref

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(32))
NKEYS, NCERTS, VOTES = 8, 128, 128
SHORT, EMPTY = 40, 77                     # certificate 40 claims 120 of its 128 votes; 77 claims none
BAD = [5, 3 * VOTES + 7, SHORT * VOTES + 125, EMPTY * VOTES + 3, 100 * VOTES, NCERTS * VOTES - 1]
MIB = 1 << 20


@pytest.fixture(scope="module")
def eng():
    from narwhal_amd import _lib
    e = _lib.Engine(device=0, key_window=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def votes(eng):
    """16,385 votes over 8 keys (the last one is the 129th certificate's) and the strict verdict of
    each from the CPU reference, shared by both sizes."""
    from narwhal_amd import workload
    com = workload.make_committee(NKEYS, eng)
    com.stake = np.arange(1, NKEYS + 1, dtype=np.uint32)
    slots = eng.committee_load_np(com.pks, com.stake)
    msgs = workload.certificate_digests(NCERTS + 1, com, eng)
    nsigs = NCERTS * VOTES + 1
    cert_of = np.minimum(np.arange(nsigs) // VOTES, NCERTS)
    signer = ((np.arange(nsigs) * 5 + cert_of) % NKEYS).astype(np.uint32)
    _, sigs = eng.sign_many_np(com.seeds[signer], msgs[cert_of])
    sigs = sigs.copy()
    sigs[BAD, 41] ^= 2                                                   # a bit of S
    strict = np.array([nw_ref.verify_strict(bytes(com.pks[signer[v]]), bytes(msgs[cert_of[v]]), bytes(sigs[v]))
                       for v in range(nsigs)])
    assert not strict[BAD].any() and strict.sum() == nsigs - len(BAD)
    return com, slots, msgs, signer, sigs, strict


def _case(votes, extra):
    from narwhal_amd import workload
    com, slots, msgs, signer, sigs, strict = votes
    nc, ns = NCERTS + extra, NCERTS * VOTES + extra
    first = (np.arange(nc) * VOTES).astype(np.uint32)
    nv = np.full(nc, VOTES, np.uint32)
    nv[SHORT], nv[EMPTY] = VOTES - 8, 0
    if extra:
        nv[NCERTS] = 1
    cs = workload.Certificates(cert_first=first, cert_n=nv, msgs=msgs[:nc].copy(), signer=signer[:ns].copy(),
                               sigs=sigs[:ns].copy())
    return cs, strict[:ns]


@pytest.mark.parametrize("extra", [0, 1], ids=["16384-prestaged", "16385-preamble-kernels"])
def test_verify_certs_across_the_prestage_switch(eng, votes, extra):
    import torch
    com, slots = votes[0], votes[1]
    cs, strict = _case(votes, extra)
    assert cs.nsigs == 16384 + extra
    claimed = np.zeros(cs.nsigs, bool)
    for f, n in zip(cs.cert_first, cs.cert_n):
        claimed[f:f + n] = True
    assert (~claimed).sum() == 8 + VOTES
    want_ok = nw_ref.verify_certs(cs, com, list(range(cs.ncerts)), ZSEED, 8, cert_base=7)
    want_stake = [int(com.stake[cs.signer[f:f + n]][strict[f:f + n]].sum()) for f, n in zip(cs.cert_first, cs.cert_n)]
    assert not want_ok[0] and not want_ok[3] and want_ok[1] and want_ok[SHORT] and not want_ok[100]

    cert_ok, sig_ok, stake = eng.verify_certs_np(cs.cert_first, cs.cert_n, cs.sigs, slots[cs.signer], cs.msgs,
                                                 ZSEED, 7)
    assert cert_ok.astype(bool).tolist() == want_ok
    assert (sig_ok.astype(bool)[claimed] == strict[claimed]).all()
    assert stake.tolist() == want_stake

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    d = dict(sig=torch.from_numpy(cs.sigs).to(dev), signer=torch.from_numpy(slots[cs.signer].astype(np.int32)).to(dev),
             first=torch.from_numpy(cs.cert_first.astype(np.int32)).to(dev),
             n=torch.from_numpy(cs.cert_n.astype(np.int32)).to(dev), msg=torch.from_numpy(cs.msgs).to(dev))
    ok_d = torch.zeros(cs.ncerts, dtype=torch.uint8, device=dev)
    flags_d = torch.zeros(cs.nsigs, dtype=torch.int32, device=dev)
    stake_d = torch.zeros(cs.ncerts, dtype=torch.int64, device=dev)
    eng.verify_certs_dev(cs.ncerts, d["first"].data_ptr(), d["n"].data_ptr(), cs.nsigs, d["sig"].data_ptr(),
                         d["signer"].data_ptr(), d["msg"].data_ptr(), ZSEED, 7, ok_d.data_ptr(), flags_d.data_ptr(),
                         stake_d.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    assert (ok_d.cpu().numpy() == cert_ok).all()
    assert ((flags_d.cpu().numpy() & 8 != 0) == sig_ok.astype(bool)).all()
    assert (stake_d.cpu().numpy() == stake.astype(np.int64)).all()


@pytest.fixture(scope="module")
def signers(eng):
    seeds = [bytes([i + 1]) * 32 for i in range(3)]
    pks = [o.public_from_seed(s) for s in seeds]
    eng.committee_load(pks, [1, 1, 1])                                   # cached: the comb path
    return seeds, pks


@pytest.mark.parametrize("big", [2 * MIB - 8192, 2 * MIB], ids=["one-dma", "staged"])
def test_cached_calls_across_the_small_call_limit(eng, signers, big):
    seeds, pks = signers
    msgs = [b"hello", b"", bytes(np.random.default_rng(big).integers(0, 256, big, dtype=np.uint8))]
    sigs = [o.sign(s, m) for s, m in zip(seeds, msgs)]
    forged = list(sigs)
    forged[2] = sigs[2][:41] + bytes([sigs[2][41] ^ 2]) + sigs[2][42:]
    for case in (sigs, forged):
        want = [o.verify_strict(k, m, s) for k, m, s in zip(pks, msgs, case)]
        assert want == [True, True, case is sigs]
        assert eng.verify_strict_many(msgs, pks, case) == want
        want_batch = o.verify_batch_z(msgs, case, pks, o.batch_coefficients(ZSEED, 11, 3))
        assert want_batch == (case is sigs)
        assert eng.verify_batch(msgs, pks, case, ZSEED, 11) == want_batch
