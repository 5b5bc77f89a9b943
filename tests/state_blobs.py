"""State blobs built in numpy for the tests (no GPU): the header, the
STREAM_STATE_DTYPE records, carries, histories and delay lines, as
qpsk_demod_get_state lays them out."""
import numpy as np

import qpsk_amd as Q

BLOB_MAGIC, BLOB_FORMAT = 0x4B535051, 2
CARRY_MAX, FLL_TAPS = 256, 40


def fresh_records(n):
    """A new handle's records: base = 1, everything else zero."""
    rec = np.zeros(n, dtype=Q.STREAM_STATE_DTYPE)
    rec["base"] = 1
    return rec


def make_blob(rec, taps, carry=None, hist=None, delay=None, magic=BLOB_MAGIC, fmt=BLOB_FORMAT, streams=None,
              hdr_taps=None):
    n = rec.size
    hd = np.array([0, 0, streams if streams is not None else n, hdr_taps if hdr_taps is not None else taps,
                   CARRY_MAX, FLL_TAPS, Q.STREAM_STATE_DTYPE.itemsize, 0], dtype=np.int32)
    hd.view(np.uint32)[:2] = (magic, fmt)
    carry = np.zeros((n, CARRY_MAX, 2), np.float32) if carry is None else carry
    hist = np.zeros((n, taps - 1, 2), np.float32) if hist is None else hist
    delay = np.zeros((n, 2 * FLL_TAPS, 2), np.float32) if delay is None else delay
    return b"".join(a.tobytes() for a in (hd, rec, carry, hist, delay))


def bad_blob(sps, span, n_streams, stream, field, value):
    """One valid blob of n_streams fresh records with one field of one stream
    set to value."""
    rec = fresh_records(n_streams)
    rec[field][stream] = value
    return make_blob(rec, span * sps + 1)
