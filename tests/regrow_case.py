"""The job of the regrow tests (test_gpu_device_rows.py, test_gpu_device_final.py): a 300-bp read, then a 23-kb one, every
chunk a batch of its own.  The first batch sizes the job's record store (rows_batch in csrc/sd_stream.hip) to
1.25 x (chunks of the job / chunks of the batch) x the batch's records + 64; the short read's chunk holds so few records
that the long read's chunks outgrow that, so the store -- and a device-final job's identity words beside it -- is
regrown behind a later batch with records already in it."""
from stringdecomposer_amd import lib, synth

LENGTHS = [300, 23000]
MAX_BATCH_ROWS = 5600        # just above one default chunk (5500): no two chunks of the job share a batch
THREADS = 8


def monomers():
    return synth.make_monomers(12, seed=3)


def reads(ms):
    return [synth.make_reads(ms, 1, read_len=n, seed=41 + i)[1][0] for i, n in enumerate(LENGTHS)]


def n_chunks(rs):
    return sum(len(lib.chunk_plan(len(s))) for s in rs)


_checked = []


def job():
    """(monomers, reads), after the proof -- made once -- that the first sizing of the store cannot hold the job: the
    records per chunk, from an engine, against the sizing rule."""
    if not _checked:
        mono = monomers()
        rs = reads(mono[1])
        _assert_store_regrows(mono[1], rs)
        _checked.append((mono, rs))
    return _checked[0]


def _assert_store_regrows(ms, rs):
    e = lib.Engine(ms, threads=THREADS)
    try:
        e.load_reads(rs)
        e.run()
        n = [len(c) for c in e.fetch()]
    finally:
        e.close()
    assert len(n) == n_chunks(rs) and len(lib.chunk_plan(len(rs[0]))) == 1
    assert n[0] > 0, n
    assert int(n[0] * 1.25 * len(n)) + 64 < sum(n), n
