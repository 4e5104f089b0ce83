"""Two threads whose FIRST calls of the process are records_unspent_named_many, over 150 strings each: the one-time builds of the commitment table and of the
serial-number tables (host) and their uploads (device) happen under both (the account owns two of every three strings: 100 records), and one of the two builds a
spent set on the device.  Prints 'ok' when both results equal the host path's and hold the reference's commitment and serial number.  Run by
tests/test_records_commit.py with ALEO_MI355X_MIN_RECORDS=0, MIN_DECRYPT=0, MIN_SERIALS=0 and MIN_COMMITMENTS=0.  The account comes from tests/serial_ref.py
(plain Python), so that nothing of the library runs before the threads start."""
import json, os, sys, threading
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
from aleo_amd import records
import serial_ref as S

GOLDEN = os.path.join(os.path.dirname(HERE), 'golden')
REC = json.load(open(os.path.join(GOLDEN, 'reference_records.json')))
SN = json.load(open(os.path.join(GOLDEN, 'reference_serial.json')))['serial_number']


def main():
    le32 = lambda v: int(v).to_bytes(32, 'little')
    from oracle import poseidon as ps
    sk = S.account_from_private_key(SN['private_key'])[0]                                        # the reference signs with a key that is not the owner's
    view, ax = ps.view_key_scalar(REC['view_keys']['owner']), ps.address_point(REC['addresses']['owner'])[0]
    acct = records.Account(None, le32(sk), le32(view), le32(ax))
    other = records.Account(None, le32(sk + 1), le32(view), le32(ax))
    plain = S.record_decrypt_fields(REC['records']['owner'], view)
    cm = le32(S.record_commitment(REC['records']['owner'], plain, SN['program_id'], SN['record_name']))
    expected = le32(int(SN['expected'][:-5]))
    strings = [REC['records']['owner'], REC['records']['sdk_foreign'], REC['records']['sdk']] * 50
    spent = [(), [expected, le32(7), le32(7)]]
    got = [None, None]
    def work(i): got[i] = records.unspent_named_many(strings, SN['program_id'], SN['record_name'], [acct, other], spent[i])
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    for i in range(2):
        want = records.unspent_named_many(strings, SN['program_id'], SN['record_name'], [acct, other], spent[i], host=True)
        assert got[i] is not None and len(got[i]) == 2, i
        for g, w in zip(got[i], want):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(g.arrays(), w.arrays())) and g.serials.tobytes() == w.serials.tobytes() and g.owned == w.owned == 100, i
            assert g.commitments.tobytes() == w.commitments.tobytes() == cm * len(g), i
    assert got[0][0].serials.tobytes() == expected * 100 and len(got[1][0]) == 0 and len(got[1][1]) == 100 and got[0][1].serials.tobytes() == got[1][1].serials.tobytes() != expected * 100
    print('ok')


if __name__ == '__main__':
    main()
