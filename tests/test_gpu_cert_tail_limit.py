"""Either side of the k_cert_tail limit (CertPlan, nw_host_plan.h): at most 16 certificates and at
most 65,536 signatures finalize in one wave (k_cert_tail, which also sums the exact list); one more
signature takes k_cert_finalize_wg<1024> (a workgroup per certificate: more than 1,024 votes on
average) + k_cert_exact.  The same switch is k_finish<true> | k_finish<false>.

  shape A   16 certificates x 4,096 votes                     65,536 signatures
  shape B   the same, the last certificate with 4,097 votes   65,537 signatures

Certificate 3 has one vote with a changed S (one term with a prime-order component: rejected without
a scalar multiplication); certificate 9 has two votes whose R is another vote's R, a valid point
(two such terms: k_slow_mul and the exact sum run).  Certificate verdicts against the oracle's batch
equation under the same coefficients; strict verdicts against the oracle's verify_strict on every
changed vote and on the first and last vote of every certificate, the rest being honest signatures
of certificates the oracle accepts; accepted stake = the stake of the strictly valid votes.
"""
import os
import types

import numpy as np
import pytest

import nw_ref

pytestmark = pytest.mark.gpu

ZSEED = bytes(range(32))
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
NKEYS, NCERTS, VOTES = 64, 16, 4096
S_CHANGED = 3 * VOTES + 1000
R_SWAPPED = (9 * VOTES + 5, 9 * VOTES + 4000)      # each takes its neighbour's R


@pytest.fixture(scope="module")
def shapes():
    from narwhal_amd import _lib, workload
    eng = _lib.Engine(device=0)
    com = workload.make_committee(NKEYS, eng)
    com.stake = np.arange(1, NKEYS + 1, dtype=np.uint32)
    slots = np.asarray(eng.committee_load_np(com.pks, com.stake), np.uint32)
    msgs = workload.certificate_digests(NCERTS, com, eng)
    total = NCERTS * VOTES + 1                      # shape B; shape A is its first 65,536 votes
    cert_of = np.minimum(np.arange(total) // VOTES, NCERTS - 1)
    signer = ((cert_of + np.arange(total)) % NKEYS).astype(np.uint32)
    _, sigs = eng.sign_many_np(com.seeds[signer], msgs[cert_of])
    sigs[S_CHANGED, 40] ^= 1
    for v in R_SWAPPED:
        assert signer[v] != signer[v + 1]
        sigs[v, :32] = sigs[v + 1, :32]
    first = (np.arange(NCERTS, dtype=np.uint32) * VOTES).astype(np.uint32)
    yield eng, com, slots, msgs, first, cert_of, signer, sigs
    eng.close()


@pytest.mark.parametrize("extra", [0, 1], ids=["65536-k_cert_tail", "65537-k_cert_finalize_wg"])
def test_cert_tail_limit(shapes, extra):
    eng, com, slots, msgs, first, cert_of, signer, sigs = shapes
    nsigs = NCERTS * VOTES + extra
    cert_n = np.full(NCERTS, VOTES, np.uint32)
    cert_n[-1] += extra
    cs = types.SimpleNamespace(cert_first=first, cert_n=cert_n, msgs=msgs, signer=signer[:nsigs], sigs=sigs[:nsigs])
    cert_ok, sig_ok, stake = eng.verify_certs_np(first, cert_n, cs.sigs, slots[cs.signer], msgs, ZSEED, 0)
    want_cert = nw_ref.verify_certs(cs, com, list(range(NCERTS)), ZSEED, THREADS)
    assert want_cert == [c not in (3, 9) for c in range(NCERTS)]
    assert cert_ok.astype(bool).tolist() == want_cert
    changed = [S_CHANGED, *R_SWAPPED]
    want_sig = np.ones(nsigs, bool)
    want_sig[changed] = False
    probe = sorted(set(changed) | set(first.tolist()) | set((first + cert_n - 1).tolist()))
    assert [bool(want_sig[v]) for v in probe] == [
        nw_ref.verify_strict(bytes(com.pks[signer[v]]), bytes(msgs[cert_of[v]]), bytes(sigs[v])) for v in probe]
    assert (sig_ok.astype(bool) == want_sig).all(), np.flatnonzero(sig_ok.astype(bool) != want_sig)[:10]
    want_stake = np.bincount(cert_of[:nsigs], weights=com.stake[signer[:nsigs]] * want_sig, minlength=NCERTS)
    assert stake.astype(np.int64).tolist() == want_stake.astype(np.int64).tolist()
