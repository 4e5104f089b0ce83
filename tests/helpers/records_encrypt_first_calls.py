"""Two threads whose FIRST calls of the process are encrypt_many over 130 plaintext strings each: the one-time build of the table of G (host) and its upload
(device) happen under both.  Prints 'ok' when both results equal the host path's, the lanes routed exactly the structs, and the reference's plaintext came back
from the device's own decryption.  Run by tests/test_records_encrypt.py with ALEO_MI355X_MIN_ENCRYPT=0.  The strings come from the golden files alone, so that
nothing of the library runs before the threads start."""
import json, os, sys, threading
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
from aleo_amd import records

GOLDEN = os.path.join(os.path.dirname(HERE), 'golden')
REF = json.load(open(os.path.join(GOLDEN, 'reference_records.json')))
GOLD = json.load(open(os.path.join(GOLDEN, 'reference_plaintexts.json')))


def main():
    plain = REF['plaintexts']['owner']
    struct = plain.replace('microcredits: 1500000000000000u64.private', 'pair: {\n    a: 1u8.private,\n    b: 2u8.private\n  }')
    strings = ([plain] + [g['string'] for g in GOLD['plaintexts']] + [struct, GOLD['invalid']['string'], plain.replace('.private,\n  _nonce', '.public,\n  _nonce')]) * 18 + ['string'] * 4
    rs = [[1000 + 2 * i for i in range(len(strings))], [7 + 3 * i for i in range(len(strings))]]
    got, routed = [None, None], [None, None]
    def work(i): got[i] = records.encrypt_many(strings, rs[i], set_nonce=True); routed[i] = records.encrypt_last_routed()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    for i in range(2):
        want = records.encrypt_many(strings, rs[i], set_nonce=True, host=True)
        assert got[i] is not None and routed[i] == 2 * 18 + 4, (i, routed)
        assert got[i][0].text == want[0].text and got[i][0].offsets.tolist() == want[0].offsets.tolist() and got[i][1].tolist() == want[1].tolist() and got[i][2].tobytes() == want[2].tobytes(), i
    batch, flags, rvk = got[0]
    assert flags[:7].tolist() == [0, 0, 0, 0, 0, 3, 0] and flags[-4:].tolist() == [3] * 4
    found = records.decrypt_strings(batch, REF['view_keys']['owner'], REF['addresses']['owner'], host=True)
    assert 0 in found.index.tolist() and found.microcredits[0] == 1500000000000000
    print('ok')


if __name__ == '__main__':
    main()
