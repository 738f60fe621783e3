"""What the assembly generators (tools/gen_*.py, tools/experiments/gen_*.py) share: the in-order issue model that counts every
`s_waitcnt` of the generated kernels, the buffer descriptor, the packed exact GELU, and the writer of the `*_asm.inc` files.
A generator holds what is its own -- register map, schedule, accumulator layout, ablation switches -- and nothing of this.

The issue model: LDS operations return in order, and so do vector-memory operations, so "operation X has landed" = "at most as
many operations are outstanding as were issued after X".  `Emit` keeps the two queues of outstanding operations (tags, oldest
first); `need_lds` / `need_vm` turn a set of tags into the one counter value that covers them all.
"""
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pips_amd", "csrc")

# The counter fields of s_waitcnt: a queue longer than the field can say is waited down to the field's maximum.  Waiting for a
# little more than needed is correct: the operations asked for have landed all the same, and a few younger ones with them.
LGKM_MAX = 15       # lgkmcnt: 4 bits
VM_MAX = 63         # vmcnt: 6 bits


def out_path(inc_name, directory=CSRC):
    """where a generator writes: PIPS_GEN_OUT, or the committed file"""
    return os.environ.get("PIPS_GEN_OUT", os.path.join(directory, inc_name))


class Emit:
    """Instruction list + in-order issue model of the two counters."""

    def __init__(self, barriers=True):
        self.lines = []
        self.lgkm = []          # outstanding LDS operations, oldest first (tags)
        self.vm = []            # outstanding vector-memory operations
        self.barriers = barriers                              # False (timing probe): the waves of a block run unsynchronised

    def raw(self, s):
        self.lines.append(s)

    def lds(self, s, tag):
        self.lines.append(s)
        self.lgkm.append(tag)

    def vmem(self, s, tag):
        self.lines.append(s)
        self.vm.append(tag)

    def _need(self, queue, tags, counter, limit, emit):
        idx = [k for k, t in enumerate(queue) if t in tags]
        if not idx:
            return queue
        left = min(len(queue) - 1 - max(idx), limit)
        if emit:
            self.lines.append("s_waitcnt %s(%d)" % (counter, left))
        return queue[len(queue) - left:] if left else []

    def need_lds(self, tags, emit=True):
        """wait until every LDS operation in `tags` has returned (emit=False, timing probes: count the wait, leave it out)"""
        self.lgkm = self._need(self.lgkm, tags, "lgkmcnt", LGKM_MAX, emit)

    def need_vm(self, tags, emit=True):
        """the same for the vector-memory operations in `tags`"""
        self.vm = self._need(self.vm, tags, "vmcnt", VM_MAX, emit)

    def need_loads(self):
        """every load issued so far has landed (stores, tagged ("out", ..), may stay in flight)"""
        self.need_vm({t for t in self.vm if t[0] != "out"})

    def barrier(self):
        if self.lgkm:
            self.lines.append("s_waitcnt lgkmcnt(0)")
            self.lgkm = []
        if self.barriers:
            self.lines.append("s_barrier")

    def drain(self):
        """full wait: nothing outstanding on either counter"""
        self.lines.append("s_waitcnt vmcnt(0) lgkmcnt(0)")
        self.lgkm, self.vm = [], []


def descriptor(e, base, lo, hi, nrec="0x7fffffff"):
    """raw buffer resource in s[base:base+3]: 48-bit base address, stride 0, `nrec` bytes in range (reads behind them return
    zero, stores are dropped)"""
    e.raw("s_mov_b32 s%d, %s" % (base, lo))
    e.raw("s_and_b32 s%d, %s, 0xffff" % (base + 1, hi))
    e.raw("s_mov_b32 s%d, %s" % (base + 2, nrec))
    e.raw("s_mov_b32 s%d, 0x00020000" % (base + 3))


def f32(x):
    """bit pattern of a float, as an assembler literal"""
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def gelu4(e, X, T, Q, s_gc, vc, ncoef):
    """exact GELU of the 8 values v[X:X+7] in place: gelu_exact2's arithmetic (common.h) with an exponent polynomial of `ncoef`
    coefficients, four pairs side by side.  T, Q: 8 scratch registers each; s_gc: the coefficients, highest power first, one per
    even scalar register, and the clamp at s_gc + 18; v[vc:vc+1]: the second coefficient as a vector pair (an instruction
    takes ONE scalar operand)."""
    for p in range(4):
        for h in range(2):
            e.raw("v_min_f32_e64 v%d, |v%d|, s%d" % (T + 2 * p + h, X + 2 * p + h, s_gc + 18))
    for p in range(4):          # q = c0 t + c1
        e.raw("v_pk_fma_f32 v[%d:%d], v[%d:%d], s[%d:%d], v[%d:%d] op_sel_hi:[1,0,1]" %
              (Q + 2 * p, Q + 2 * p + 1, T + 2 * p, T + 2 * p + 1, s_gc, s_gc + 1, vc, vc + 1))
    for c in range(2, ncoef):
        for p in range(4):
            e.raw("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], s[%d:%d] op_sel_hi:[1,1,0]" %
                  (Q + 2 * p, Q + 2 * p + 1, Q + 2 * p, Q + 2 * p + 1, T + 2 * p, T + 2 * p + 1, s_gc + 2 * c, s_gc + 2 * c + 1))
    for p in range(4):
        e.raw("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (Q + 2 * p, Q + 2 * p + 1, Q + 2 * p, Q + 2 * p + 1, T + 2 * p, T + 2 * p + 1))
    for p in range(4):
        for h in range(2):
            e.raw("v_exp_f32_e32 v%d, v%d" % (Q + 2 * p + h, Q + 2 * p + h))
    for p in range(4):
        for h in range(2):
            e.raw("v_max_f32_e32 v%d, 0, v%d" % (X + 2 * p + h, X + 2 * p + h))
    for p in range(4):
        e.raw("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (T + 2 * p, T + 2 * p + 1, T + 2 * p, T + 2 * p + 1, Q + 2 * p, Q + 2 * p + 1))
    for p in range(4):
        e.raw("v_pk_fma_f32 v[%d:%d], v[%d:%d], -0.5, v[%d:%d] op_sel_hi:[1,0,1]" %
              (X + 2 * p, X + 2 * p + 1, T + 2 * p, T + 2 * p + 1, X + 2 * p, X + 2 * p + 1))


def write_inc(out, generator, bodies, clobber_name, n_acc, n_vgpr, sgprs, notes=()):
    """The .inc file of `generator`: per (macro name, lines) of `bodies` one string-literal #define, one instruction per line,
    then the clobber macro: memory, scc, vcc, a[0:n_acc], v[0:n_vgpr] and the scalar registers of the range `sgprs`.  Prints
    one statistics line per body, with the matching entry of `notes` behind it."""
    clob = ['"memory"', '"scc"', '"vcc"'] + ['"a%d"' % i for i in range(n_acc)] + ['"v%d"' % i for i in range(n_vgpr)] + \
           ['"s%d"' % i for i in sgprs]
    with open(out, "w") as f:
        f.write("// generated by tools/%s -- do not edit\n" % generator)
        for k, (name, lines) in enumerate(bodies):
            f.write("#define %s \\\n" % name)
            for ln in lines:
                f.write('    "%s\\n\\t" \\\n' % ln)
            f.write('    ""\n\n')
            print("%s: %d instructions, %d MFMAs" % (name, len(lines), sum("v_mfma" in ln for ln in lines)) + (notes[k] if notes else ""))
        f.write("#define %s " % clobber_name + ", ".join(clob) + "\n")
    print("wrote", out)
