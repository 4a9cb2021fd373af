"""ParseAdfea (difacto_amd/host/reader.cc; src/reader/adfea_parser.h:34-84) restated in Python,
byte by byte: whitespace-separated tokens; "idx:gid" is a feature (idx << 12) | (gid & 4095),
every other token that starts with a digit cycles lineid, count, label, and the label opens a new
row and is 1 iff it starts with '1'.  idx and gid are strtoull's: leading digits, saturating at
2^64 - 1; the shift wraps mod 2^64.  The device parser (csrc/adfeaparse.hip) is tested against the
C++ original; this restatement holds the known answers and the property its domain rests on."""
import re

M64 = (1 << 64) - 1
SPACE = b" \t\n\r"
DIGIT = b"0123456789"

# the lines dfx_parse_adfea parses on the device
CONFORMING = re.compile(rb"[ \t]*\d+[ \t]+\d+[ \t]+\d+(?:[ \t]+\d+:\d+)*[ \t]*\n")


def strtoull(data, p):
    """strtoull(data + p, NULL, 10) on a text that starts with a digit or not at all"""
    v, q = 0, p
    while q < len(data) and data[q] in DIGIT:
        v = v * 10 + (data[q] - 48)
        q += 1
    return min(v, M64)


def parse(data):
    """-> (offsets, ids, labels) of ParseAdfea(data, data + len(data)) into an empty block"""
    data = bytes(data)
    e = len(data)
    offsets, ids, labels = [0], [], []
    i = p = 0
    while p != e and data[p] in SPACE:
        p += 1
    while p != e:
        head = p
        while p != e and data[p] in DIGIT:
            p += 1
        if head == p:  # not a number: skip the token
            while p != e and data[p] not in SPACE:
                p += 1
        elif p != e and data[p] == ord(":"):
            p += 1
            idx, gid = strtoull(data, head), strtoull(data, p)
            if labels:
                ids.append(((idx << 12) & M64) | (gid & 4095))
            while p != e and data[p] in DIGIT:
                p += 1
        elif i == 2:
            i = 0
            if labels:
                offsets.append(len(ids))
            labels.append(1.0 if data[head] == ord("1") else 0.0)
        else:
            i += 1
        while p != e and data[p] in SPACE:
            p += 1
    if labels:
        offsets.append(len(ids))
    return offsets, ids, labels


def concat(parts):
    """the blocks of the pieces of a chunk, concatenated in order (the host's ConcatParts)"""
    offsets, ids, labels = [0], [], []
    for off, idx, lab in parts:
        offsets.extend(len(ids) + o for o in off[1:])
        ids.extend(idx)
        labels.extend(lab)
    return offsets, ids, labels


def conforming(data):
    """every line of data is in the device's domain, the last one terminated"""
    data = bytes(data)
    pos = 0
    while pos < len(data):
        m = CONFORMING.match(data, pos)
        if not m:
            return False
        pos = m.end()
    return True
