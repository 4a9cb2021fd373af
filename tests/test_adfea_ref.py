"""The CPU half of the device adfea parser's tests: ParseAdfea restated (tests/adfea_ref.py) with
its known answers, the id edges and the property the device's domain rests on (for conforming
text the host's result does not depend on where the chunk is cut at newlines), the generator's
rows being inside that domain, and the batch planner on binary rows of varying length against
BatchReader (tests/host/adfeaparse_tests.cc, mode plan).  No HIP call."""
import os
import random
import subprocess

from tests import adfea_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "build", "gen_adfea")
BIN = os.path.join(ROOT, "build", "adfeaparse_tests")

SAMPLE = b"1 3 1 17:2 123456789:4095 5:1\n2 1 0 9:7\n3 0 1\n"


def _make(*targets):
    subprocess.check_call(["make", "-s"] + list(targets), cwd=ROOT)


def test_known_answer_of_the_host_reader_test():
    """the three rows tests/host/reader_tests.cc pins for ParseAdfea"""
    offsets, ids, labels = A.parse(SAMPLE)
    assert labels == [1.0, 0.0, 1.0]
    assert offsets == [0, 3, 4, 4]
    assert ids[:3] == [(17 << 12) | 2, (123456789 << 12) | 4095, (5 << 12) | 1]
    assert ids[3] == (9 << 12) | 7
    assert A.conforming(SAMPLE)
    assert A.parse(b"") == ([0], [], []) and A.parse(b"7 0 1\n") == ([0, 0], [], [1.0])


def test_id_edges():
    """idx: 0, leading zeros, 2^52 - 1, 2^52 (the shift wraps), 2^64 - 1, 2^64 and 25 digits (both
    saturate); gid: 0, 4095, 4096 (-> 0), 2^64 (-> 4095)"""
    def one(tok):
        return A.parse(b"1 1 1 " + tok + b"\n")[1][0]
    assert one(b"0:0") == 0
    assert one(b"000017:0004095") == (17 << 12) | 4095
    assert one(b"%d:4095" % (2 ** 52 - 1)) == A.M64
    assert one(b"%d:4096" % 2 ** 52) == 0
    assert one(b"%d:1" % (2 ** 64 - 1)) == (A.M64 << 12) & A.M64 | 1
    assert one(b"%d:%d" % (2 ** 64, 2 ** 64)) == (A.M64 << 12) & A.M64 | 4095
    assert one(b"1234567890123456789012345:7") == (A.M64 << 12) & A.M64 | 7
    assert one(b"9:0") == 9 << 12


def test_labels_follow_the_first_byte():
    text = b"".join(b"%d 0 %s\n" % (i, lab) for i, lab in
                    enumerate([b"1", b"0", b"10", b"01", b"2", b"1234567890123"]))
    assert A.parse(text)[2] == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]


def _random_conforming(rng, rows):
    blank = lambda lo=1: "".join(rng.choice(" \t") for _ in range(rng.randint(lo, 3)))  # noqa
    out = []
    for r in range(rows):
        nnz = rng.randint(0, 5)
        line = blank(0) + str(r) + blank() + str(nnz) + blank() + rng.choice(["0", "1", "10", "7"])
        for _ in range(nnz):
            line += blank() + "%d:%d" % (rng.getrandbits(rng.choice([8, 30, 64])),
                                         rng.randrange(5000))
        out.append(line + blank(0) + "\n")
    return "".join(out).encode()


def test_conforming_text_parses_the_same_wherever_it_is_cut_at_newlines():
    """the property the device's domain rests on: TextReader::ParseChunk cuts a chunk at
    newlines for its threads and concatenates; for conforming text (the parser's token counter is
    back at 0 after every line) that equals parsing the chunk whole, at every single cut and at
    random sets of cuts"""
    rng = random.Random(20261021)
    text = _random_conforming(rng, 60)
    assert A.conforming(text)
    whole = A.parse(text)
    assert len(whole[2]) == 60 == text.count(b"\n")
    cuts = [i + 1 for i, c in enumerate(text) if c == 10]
    for c in cuts:
        assert A.concat([A.parse(text[:c]), A.parse(text[c:])]) == whole, c
    for _ in range(50):
        pick = sorted(rng.sample(cuts, rng.randint(2, 7)))
        edges = [0] + pick + [len(text)]
        parts = [A.parse(text[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        assert A.concat(parts) == whole, pick


def test_a_continued_row_depends_on_the_cut():
    """a row continued on the next line (which the host accepts and the device flags) is outside
    the domain: the piece after the cut drops the continuation's features, so the equality
    fails"""
    text = b"1 2 1 5:1\n6:2\n2 1 0 7:3\n"
    assert not A.conforming(text)
    whole = A.parse(text)
    assert whole == ([0, 2, 3], [(5 << 12) | 1, (6 << 12) | 2, (7 << 12) | 3], [1.0, 0.0])
    c = text.index(b"\n") + 1
    assert A.concat([A.parse(text[:c]), A.parse(text[c:])]) != whole
    for bad in (b"\n", b"1 2\n", b"1 2 1 5\n", b"1 5:1 1\n", b"1 2 1 5:1\r\n", b"1 2 1 5:1"):
        assert not A.conforming(bad), bad


def test_generated_rows_conform(tmp_path):
    """build/gen_adfea writes rows inside the device's domain, with mixed blanks, the asked row
    lengths and ids"""
    _make("build/gen_adfea")
    path = tmp_path / "g.adfea"
    subprocess.check_call([GEN, str(path), "500", "3", "0", "9", "64", "4096"])
    text = path.read_bytes()
    assert A.conforming(text) and b"\t" in text and b"  " in text
    offsets, ids, labels = A.parse(text)
    assert len(labels) == 500 and 0 < sum(labels) < 500
    lens = {b - a for a, b in zip(offsets[:-1], offsets[1:])}
    assert min(lens) == 0 and max(lens) == 9
    assert max(i & 4095 for i in ids) > 39 and max(ids) >> 60
    again = tmp_path / "g2.adfea"
    subprocess.check_call([GEN, str(again), "500", "3", "0", "9", "64", "4096"])
    assert again.read_bytes() == text


def test_planner_on_binary_rows_of_varying_length(tmp_path):
    """BatchPlanner fed the host-parsed adfea chunks' lengths and labels, its plan carried out
    with host GatherRows: the batches equal BatchReader's (5,000 rows of 5-15 features, batch 257,
    64 KB chunks, shuffle 0 / 3, neg_sampling 1 / 0.7, parts 0/1 and 1/2).  No HIP call."""
    _make("build/gen_adfea", "build/adfeaparse_tests")
    data = tmp_path / "rows.adfea"
    subprocess.check_call([GEN, str(data), "5000", "7", "5", "15", "24", "39"])
    r = subprocess.run([BIN, "plan", str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("batches ok") == 8
