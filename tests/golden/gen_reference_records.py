#!/usr/bin/env python3
"""Generates reference_records.json: the DATA the reference's own tests hold about record ciphertexts and their owners.

  wasm/src/record/record_ciphertext.rs:91-137   a record ciphertext, its owner's view key and address, a non-owner's view key, the plaintext (with
                                                the `_nonce` literal), the two strings test_invalid_strings refuses, and the booleans test_is_owner asserts
  sdk/tests/data/account-data.ts:13-27          the same record, a foreign ciphertext and a foreign view key; sdk/tests/wasm.test.ts:337-349 asserts isOwner

Strings and booleans only; needs /root/reference.  Run from the repo root:  python tests/golden/gen_reference_records.py"""
import json, os, re
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def main():
    rs_path, ts_path = 'wasm/src/record/record_ciphertext.rs', 'sdk/tests/data/account-data.ts'
    if not os.path.exists(os.path.join(REF, rs_path)):
        print('skip reference_records.json (no /root/reference)'); return
    rs = open(os.path.join(REF, rs_path)).read()
    ts = open(os.path.join(REF, ts_path)).read()
    test = open(os.path.join(REF, 'sdk/tests/wasm.test.ts')).read()
    const = lambda name: re.search(r'const _?' + name + r': &str = r?"([^"]*)"', rs, flags=re.S).group(1)
    tsv = lambda name: re.search(r'const ' + name + r'\s*=\s*"((?:[^"\\]|\\.)*)"', ts).group(1).replace('\\n', '\n')
    plaintext = const('OWNER_PLAINTEXT')
    # what the reference asserts: test_is_owner (owner key true, the other key false); wasm.test.ts (viewKey true, foreignViewKey false)
    assert re.search(r'assert!\(record\.is_owner\(&view_key\)\)', rs) and re.search(r'assert!\(!record\.is_owner\(&incorrect_view_key\)\)', rs)
    assert re.search(r'isOwner = ciphertext\.isOwner\(viewKey\)', test) and 'expect(isOwner).toBe(true)' in test and 'expect(ciphertext.isOwner(foreignViewKey)).toBe(false)' in test
    out = {
        'sources': [rs_path + ':91-137', ts_path + ':13-27', 'sdk/tests/wasm.test.ts:337-349'],
        'records': {'owner': const('OWNER_CIPHERTEXT'), 'sdk': tsv('recordCiphertextString'), 'sdk_foreign': tsv('foreignCiphertextString')},
        'plaintexts': {'owner': plaintext, 'sdk': tsv('recordPlaintextString')},
        'nonces': {'owner': re.search(r'_nonce: (\d+)group', plaintext).group(1), 'sdk': re.search(r'_nonce: (\d+)group', tsv('recordPlaintextString')).group(1)},
        'view_keys': {'owner': const('OWNER_VIEW_KEY'), 'non_owner': const('NON_OWNER_VIEW_KEY'), 'sdk': tsv('viewKeyString'), 'sdk_foreign': tsv('foreignViewKeyString')},
        'addresses': {'owner': const('OWNER_ADDRESS'), 'sdk': tsv('addressString')},
        # (record, view key, the address of that view key's account when the reference holds it, what the reference's test asserts)
        'is_owner': [
            {'source': rs_path + ':131-137', 'record': 'owner', 'view_key': 'owner', 'address': 'owner', 'expected': True},
            {'source': rs_path + ':131-137', 'record': 'owner', 'view_key': 'non_owner', 'address': None, 'expected': False},
            {'source': 'sdk/tests/wasm.test.ts:337-342', 'record': 'sdk', 'view_key': 'sdk', 'address': 'sdk', 'expected': True},
            {'source': 'sdk/tests/wasm.test.ts:346-349', 'record': 'sdk', 'view_key': 'sdk_foreign', 'address': None, 'expected': False},
        ],
        'invalid': {'invalid_bech32': re.search(r'let invalid_bech32 = "(\w+)"', rs).group(1), 'garbage': re.search(r'from_string\("(garbage)"\)', rs).group(1)},
    }
    json.dump(out, open(os.path.join(HERE, 'reference_records.json'), 'w'), indent=1)
    print('wrote reference_records.json')


if __name__ == '__main__':
    main()
