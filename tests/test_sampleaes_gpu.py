"""SAMPLE-AES decryption on the MI355X (``kernels/sample_aes.hip``): the same cases as
``test_sampleaes.py`` through the same helpers.  The ES buffer with its canaries, the NAL rows and
``sainfo`` equal the independent reference and the host implementation bit for bit; the remux of
the decrypted batch equals the remux of the clear twin; damaged rows stay inside the selected
extents; the dispatcher op agrees with the pybind entry; misaligned offsets are rejected on the
host.  Every batch is at most a few hundred KB."""
import numpy as np
import pytest
import torch

import sampleaes_cases as sc
from hlsjs_p2p_wrapper_amd.ops import aes, sampleaes
from hlsjs_p2p_wrapper_amd.ops._native import device
from test_sampleaes import check_case_facts, check_damaged, decrypt_and_compare, end_to_end

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_cases_match_the_reference_and_the_host(name, cuda):
    assert device().sample_aes_round_bytes() == sc.ROUND == sampleaes.sample_aes_round_bytes()
    b, sa = decrypt_and_compare(name, cuda)
    assert sa.sainfo.is_cuda
    (res, caps, ix), keys, ivs, enable = sc.batch(name)[1:5]
    host = sampleaes.sample_decrypt_batch(res, ix, caps, keys, ivs, enable)
    assert torch.equal(b[1][0].es.cpu(), res.es) and torch.equal(b[1][2].nal.cpu(), ix.nal)
    assert torch.equal(sa.sainfo.cpu(), host.sainfo)


def test_case_facts(cuda):
    check_case_facts(cuda)


@pytest.mark.parametrize("name", ["video", "long", "audio", "mixed"])
def test_remux_of_the_decrypted_batch_equals_the_clear_twins(name, cuda):
    assert end_to_end(name, cuda) >= 2


def test_damaged_rows_stay_inside_the_selected_extents(cuda):
    check_damaged(cuda)


def test_dispatcher_op_agrees_with_the_pybind_entry(cuda):
    outs = []
    for op in (device().sample_aes_decrypt, torch.ops.hlsp2p.sample_aes_decrypt):
        (res, caps, ix), keys, ivs, _ = sc.batch("video", cuda)[1:5]
        want_es, want_nal, want_sainfo = sc.ref_batch(res, ix, caps, keys, ivs)
        B, max_pes, max_nal = len(caps), int(res.pes.shape[2]), int(ix.nal.shape[1])
        dev = lambda a: torch.from_numpy(np.array(a)).to(cuda)  # noqa: E731
        drk = dev(np.stack([aes.round_keys_le(k) for k in keys]).view(np.int32))
        iv = dev(np.frombuffer(b"".join(ivs), np.uint8).reshape(B, 16))
        tdl, isb = aes.device_tables(cuda)
        sainfo = torch.full((B * sampleaes.SAINFO_WORDS + 4,), -7, dtype=torch.int64, device=cuda)
        op(res.es, dev(np.asarray(res.es_offs, np.int64)), dev(np.asarray(caps, np.int64)), res.info, res.pes, max_pes,
           max_nal, ix.nal, ix.au, ix.aframes, ix.sinfo, drk, iv, dev(np.ones(B, np.uint8)), tdl, isb, sainfo)
        assert sainfo[-4:].tolist() == [-7] * 4
        assert np.array_equal(sainfo[:-4].cpu().numpy().reshape(B, -1), want_sainfo)
        assert np.array_equal(res.es.cpu().numpy(), want_es) and np.array_equal(ix.nal.cpu().numpy(), want_nal)
        outs.append(res.es.cpu())
    assert torch.equal(outs[0], outs[1])


def test_misaligned_offsets_and_short_outputs_are_rejected_on_the_host(cuda):
    (res, caps, ix), keys, ivs, _ = sc.batch("tiny", cuda)[1:5]
    before = res.es.cpu()
    res.es_offs = res.es_offs + 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        sampleaes.sample_decrypt_batch(res, ix, caps, keys, ivs)
    res.es_offs = res.es_offs - 8
    with pytest.raises(ValueError, match="one device"):
        sampleaes.sample_decrypt_batch(res, sc.batch("tiny")[1][2], caps, keys, ivs)
    torch.cuda.synchronize()
    assert torch.equal(res.es.cpu(), before)
