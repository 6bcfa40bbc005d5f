"""The reference of the record splitter (include/hypergen_rec.h), pure Python, written from the specification and calling
nothing of the library: the lines of a text, which of them are headers, the records, their identifiers, and the device layout
of the sequences with its pads.  Every test of libhypergen_rec.so compares against it with `==`."""
from collections import namedtuple

import numpy as np

Record = namedtuple("Record", "hdr_off hdr_len id_len seq")  # seq: bytes
REC_DTYPE = np.dtype([("hdr_off", np.uint64), ("hdr_len", np.uint32), ("id_len", np.uint32), ("seq_off", np.uint64),
                      ("seq_len", np.uint64)])


class SequenceBeforeHeader(ValueError):
    """a non-header line with non-empty content before the first header: HG_ERR_IO"""


def lines(text):
    """(offset, content) of every line: lines end at LF, the last may lack one; the content is the line without its LF and
    without one CR directly before the LF -- or, for an unterminated last line, as the very last byte of the text"""
    text = bytes(text)
    out, i, n = [], 0, len(text)
    while i < n:
        j = text.find(b"\n", i)
        end = n if j < 0 else j
        content = text[i:end]
        if content.endswith(b"\r"):
            content = content[:-1]
        out.append((i, content))
        i = end + 1
    return out


def split(text):
    """the records of a text, in order"""
    recs, parts = [], None
    for off, content in lines(text):
        if content.startswith(b">"):
            if parts is not None:
                recs[-1] = recs[-1]._replace(seq=b"".join(parts))
            ident = 0
            while 1 + ident < len(content) and content[1 + ident] > 0x20:
                ident += 1
            recs.append(Record(off, len(content), ident, b""))
            parts = []
        elif content:
            if parts is None:
                raise SequenceBeforeHeader()
            parts.append(content)
    if parts is not None:
        recs[-1] = recs[-1]._replace(seq=b"".join(parts))
    return recs


def layout(recs):
    """(record table, sequence buffer of seq_bytes bytes): offsets are multiples of 4, the gaps hold 'N'"""
    table = np.zeros(len(recs), REC_DTYPE)
    buf = bytearray()
    for r, rec in enumerate(recs):
        table[r] = (rec.hdr_off, rec.hdr_len, rec.id_len, len(buf), len(rec.seq))
        buf += rec.seq
        buf += b"N" * (-len(buf) % 4)
    return table, np.frombuffer(bytes(buf), np.uint8)


def merged(recs):
    """what read_merge_seq makes of the same file: 'N' + sequence per record"""
    return b"".join(b"N" + rec.seq for rec in recs)


def identifiers(text, recs):
    text = bytes(text)
    return [text[r.hdr_off + 1:r.hdr_off + 1 + r.id_len] for r in recs]
