"""tools/rocpd_sequence.py over every forward of a trace: the encoder's launch sequence (last stem convolution of a forward up to the
first gather) out of a rocprofv3 --kernel-trace rocpd database, with the mean / min / max duration per launch position over the
forwards after the first `skip` (warm-up) whose sequence equals the last one's.
usage: python tools/rocpd_sequence_avg.py <results.db> <out.txt> [skip=3]"""
import re
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
skip = int(sys.argv[3]) if len(sys.argv) > 3 else 3
rows = None
objs = [r[0] for r in db.execute("select name from sqlite_master where type in ('table','view')")]
for obj in sorted(objs, key=lambda n: (0 if n == "kernels" else 1, n)):
    cols = [c[1] for c in db.execute("pragma table_info('%s')" % obj)]
    if {"name", "start", "end"} <= set(cols):
        rows = list(db.execute("select name, start, end from '%s' order by start" % obj))
        break
if rows is None:
    print("no table with (name, start, end); objects:", objs)
    sys.exit(1)


def short(n):
    return re.sub(r"\(.*", "", n).replace("pips::", "").replace("void ", "")


stems = [i for i, r in enumerate(rows) if "stem_conv" in r[0]]
seqs = []
for i0 in stems:
    seq = []
    for name, s, e in rows[i0:]:
        if "mixer_input" in name and len(seq) > 1:
            break
        if "stem_conv" in name and len(seq) > 1:
            break
        seq.append((short(name), (e - s) / 1e3))
    seqs.append(seq)
last = [n for n, _ in seqs[-1]]
good = [s for s in seqs[skip:] if [n for n, _ in s] == last]
out = ["# %d forwards (of %d traced, first %d skipped); per launch: mean  min  max (us)" % (len(good), len(seqs), skip)]
tot = [0.0] * len(good)
for k, n in enumerate(last):
    d = [s[k][1] for s in good]
    for j, x in enumerate(d):
        tot[j] += x
    out.append("%-70s %8.1f %8.1f %8.1f" % (n[:70], sum(d) / len(d), min(d), max(d)))
out.append("%-70s %8.1f %8.1f %8.1f" % ("# encoder kernel time", sum(tot) / len(tot), min(tot), max(tot)))
txt = "\n".join(out)
print("\n".join(out[:24]))
print(out[-1])
open(sys.argv[2], "w").write(txt + "\n")
