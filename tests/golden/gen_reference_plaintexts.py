#!/usr/bin/env python3
"""Generates reference_plaintexts.json: the RecordPlaintext STRINGS the reference holds, as data.

  wasm/src/record/record_plaintext.rs:113-117   RECORD: the string of its to/from-string, microcredits (1500000000000000) and serial-number tests
  rust/src/test_utils/mod.rs:132-136            RECORD_2000000001_MICROCREDITS
  rust/src/test_utils/mod.rs:138-142            RECORD_5_MICROCREDITS
  wasm/src/record/record_plaintext.rs:175       the string from_string must refuse (an address under the prefix aleo2), and :178 the text it refuses "string" with

Strings only; needs a checkout of the reference.  Run from the repo root:  python tests/golden/gen_reference_plaintexts.py <path to the reference>"""
import json, os, re, sys
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ALEO_REFERENCE', '')
    rs_path, tu_path = 'wasm/src/record/record_plaintext.rs', 'rust/src/test_utils/mod.rs'
    if not os.path.exists(os.path.join(ref, rs_path)):
        print('skip reference_plaintexts.json (no reference checkout given)'); return
    rs, tu = open(os.path.join(ref, rs_path)).read(), open(os.path.join(ref, tu_path)).read()

    def raw(src, name): return re.search(r'const %s: &str = r"(.*?)";' % name, src, flags=re.S).group(1)
    def lines(src, text): at = src.index(text); first = src[:at].count('\n') + 1; return '%d-%d' % (first, first + text.count('\n'))
    record, two, five = raw(rs, 'RECORD'), raw(tu, 'RECORD_2000000001_MICROCREDITS'), raw(tu, 'RECORD_5_MICROCREDITS')
    invalid = re.search(r'let invalid_bech32 = "([^"]*)";', rs).group(1)
    message = re.search(r'from_string\("string"\)\.err\(\),\s*Some\("([^"]*)"', rs).group(1)
    out = {
        'plaintexts': [
            {'name': 'RECORD', 'source': rs_path + ':' + lines(rs, record), 'string': record, 'microcredits': int(re.search(r'record\.microcredits\(\), (\d+)\)', rs).group(1))},
            {'name': 'RECORD_2000000001_MICROCREDITS', 'source': tu_path + ':' + lines(tu, two), 'string': two, 'microcredits': 2000000001},
            {'name': 'RECORD_5_MICROCREDITS', 'source': tu_path + ':' + lines(tu, five), 'string': five, 'microcredits': 5},
        ],
        'invalid': {'source': rs_path + ':' + lines(rs, invalid), 'string': invalid},
        'invalid_message': {'source': rs_path + ':' + lines(rs, message), 'string': 'string', 'message': message},
    }
    json.dump(out, open(os.path.join(HERE, 'reference_plaintexts.json'), 'w'), indent=1)
    print('wrote reference_plaintexts.json')


if __name__ == '__main__':
    main()
