"""A process whose FIRST device calls come in an order no other test has: signatures_verify on 65 signatures, unspent_named_many on 102 strings (70 of them the
first two accounts') for three accounts with a spent set, serial_numbers on 65 commitments, decrypt_strings on the same strings.  The tables resident on the device
are then uploaded in the order signature, serial number, records constants, commitment, all of them before the first plain scan, and the first call that
touches the slot's pinned words is the one that reads all three groups of them (the flow's, the unspent stage's, the routed count).  Prints 'ok' when every result equals the host path's byte
for byte.  Run by tests/test_records_commit.py with every ALEO_MI355X_MIN_* at 0; the host results are computed after the four device calls."""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
from aleo_amd import records, signature as sg
import serial_ref as S

GOLDEN = os.path.join(os.path.dirname(HERE), 'golden')
REC = json.load(open(os.path.join(GOLDEN, 'reference_records.json')))
SN = json.load(open(os.path.join(GOLDEN, 'reference_serial.json')))['serial_number']


def same(got, want):
    return (all(x.tobytes() == y.tobytes() for x, y in zip(got.arrays(), want.arrays())) and got.owned == want.owned and got.unparsed == want.unparsed
            and (got.serials is None) == (want.serials is None) and (got.serials is None or got.serials.tobytes() == want.serials.tobytes())
            and (got.commitments is None) == (want.commitments is None) and (got.commitments is None or got.commitments.tobytes() == want.commitments.tobytes()))


def main():
    le32 = lambda v: int(v).to_bytes(32, 'little')
    from oracle import poseidon as ps
    signer = records.Account.from_private_key(SN['private_key'])                                 # host calls: the account, and signing
    msgs = [bytes((7 * i + j) & 255 for j in range(i)) for i in range(65)]                         # 0 .. 64 bytes
    sigs = [signer.sign(m, le32(1000 + i)).raw for i, m in enumerate(msgs)]
    sigs[3] = sigs[3][:40] + bytes([sigs[3][40] ^ 1]) + sigs[3][41:]                               # does not verify
    sigs[64] = b'\xff' * 128                                                                       # no signature
    sig_rows = np.frombuffer(b''.join(sigs), dtype=np.uint8).reshape(-1, 128)

    view, ax = ps.view_key_scalar(REC['view_keys']['owner']), ps.address_point(REC['addresses']['owner'])[0]
    sk = int.from_bytes(signer.sk_sig, 'little')
    accounts = [records.Account(None, le32(sk), le32(view), le32(ax)), records.Account(None, le32(sk + 1), le32(view), le32(ax)),
                records.Account(None, le32(sk + 2), le32(view + 1), le32(ax))]                      # the third owns nothing: an empty segment
    strings = []
    for i in range(70): strings += [REC['records']['owner']] + [REC['records']['sdk_foreign']] * (i < 32)      # 102 strings, 70 of them the first two accounts'
    batch = records.RecordBatch.from_strings(strings)
    spent = [le32(int(SN['expected'][:-5])), le32(7)]                                              # every record of the first account is spent
    plain = S.record_decrypt_fields(REC['records']['owner'], view)
    cm = le32(S.record_commitment(REC['records']['owner'], plain, SN['program_id'], SN['record_name']))
    cms = [bytes([i]) + cm[1:31] + b'\0' for i in range(65)]                                       # below 2^248: canonical

    flags = sg.verify_many(sig_rows, signer.address_x, msgs)                                       # the first four device calls of the process
    unspent = records.unspent_named_many(batch, SN['program_id'], SN['record_name'], accounts, spent)
    sn, sn_flags = records.serial_numbers(cms, signer.sk_sig)
    found = records.decrypt_strings(batch, le32(view), le32(ax))

    want_flags = sg.verify_many(sig_rows, signer.address_x, msgs, host=True)
    assert flags.tobytes() == want_flags.tobytes() and flags.tolist() == [0, 0, 0, 1] + [0] * 60 + [3], flags.tolist()
    want = records.unspent_named_many(batch, SN['program_id'], SN['record_name'], accounts, spent, host=True)
    assert len(unspent) == 3 and all(same(g, w) for g, w in zip(unspent, want))
    assert [u.owned for u in unspent] == [70, 70, 0] and [len(u) for u in unspent] == [0, 70, 0], ([u.owned for u in unspent], [len(u) for u in unspent])
    want_sn, want_sn_flags = records.serial_numbers(cms, signer.sk_sig, host=True)
    assert sn.tobytes() == want_sn.tobytes() and sn_flags.tobytes() == want_sn_flags.tobytes() and not sn_flags.any()
    assert same(found, records.decrypt_strings(batch, le32(view), le32(ax), host=True)) and len(found) == 70
    print('ok')


if __name__ == '__main__':
    main()
