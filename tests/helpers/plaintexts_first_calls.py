"""Two threads whose FIRST calls of the process are plaintext_serial_numbers over 130 plaintext strings each: the one-time builds of the commitment table and of the
serial-number tables (host) and their uploads (device) happen under both, and one of the two builds a spent set on the device.  Prints 'ok' when both results
equal the host path's and hold the reference's serial number.  Run by tests/test_plaintexts.py with ALEO_MI355X_MIN_PLAINTEXTS=0.  The key comes from
tests/serial_ref.py (plain Python), so that nothing of the library runs before the threads start."""
import json, os, sys, threading
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
from aleo_amd import records
import serial_ref as S

GOLDEN = os.path.join(os.path.dirname(HERE), 'golden')
GOLD = json.load(open(os.path.join(GOLDEN, 'reference_plaintexts.json')))
SN = json.load(open(os.path.join(GOLDEN, 'reference_serial.json')))['serial_number']


def main():
    le32 = lambda v: int(v).to_bytes(32, 'little')
    sk = le32(S.account_from_private_key(SN['private_key'])[0])
    expected = le32(int(SN['expected'][:-5]))
    strings = ([g['string'] for g in GOLD['plaintexts']] + [GOLD['invalid']['string']] * 2 + [GOLD['plaintexts'][0]['string'].replace('u64', '_0u64')] + [g['string'] for g in GOLD['plaintexts']] * 2) * 10 + ['string'] * 10
    spent = [(), [expected, le32(7), le32(7)]]
    got, routed = [None, None], [None, None]
    def work(i): got[i] = records.plaintext_serial_numbers(strings, SN['program_id'], SN['record_name'], sk, spent[i]); routed[i] = records.plaintexts_last_routed()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    for i in range(2):
        want = records.plaintext_serial_numbers(strings, SN['program_id'], SN['record_name'], sk, spent[i], host=True)
        assert got[i] is not None and routed[i] == 40, (i, routed)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[i], want)), i
    sn, cm, mc, flags = got[0]
    assert sn[0].tobytes() == expected and flags[:6].tolist() == [0, 0, 0, 3, 3, 0] and got[1][3][:6].tolist() == [1, 0, 0, 3, 3, 0] and mc[:6].tolist() == [1500000000000000, 2000000001, 5, 0, 0, 15000000000000000]
    print('ok')


if __name__ == '__main__':
    main()
