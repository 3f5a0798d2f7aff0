"""Which fp32 product-sums of a kernel ended up fused (fma) and which rounded (mul, then add)?

Walks one kernel of a hipcc -S assembly file linearly (control flow ignored: both sides of a branch are
evaluated in file order), tracks every VGPR as an expression tree over v_mul / v_add / v_sub / v_fma / v_fmac and
their packed forms, and prints, for every value that reaches a buffer store, an LDS write or a v_perm_b32, the
SHAPE of its arithmetic (leaves that are loads, MFMA results, selects or DPP moves print as _), with counts.
Under -ffp-contract=fast the compiler decides per expression -- and, after SLP vectorisation, per tile of an
unrolled loop -- whether a product is fused into the neighbouring add; two kernels that must agree bitwise have to
show the same shapes (lstmf_fwds_kernel against lstmf_fwds2_kernel: profiles/fwd_two_wave/README.md).

    python scripts/isa_fp_forms.py lstm_f32.s 17lstmf_fwds_kernelILi2ELi32ELb1ELb0E [max chars per shape]
"""
import collections
import re
import sys

def kern(path, pat):
    lines=open(path).read().split('\n')
    st=[i for i,l in enumerate(lines) if re.match(r'^_ZN5hfrep\w*'+pat+r'\w*:', l)][0]
    en=next(i for i in range(st,len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[st], lines[st+1:en]

ARITH = {'mul','add','sub','fma'}
class Sym:
    def __init__(s):
        s.r = {}; s.n = 0; s.out = []
    def fresh(s, tag):
        s.n += 1; return (tag + str(s.n),)
    def get(s, op):
        op = op.strip()
        neg = False; ab = False
        if op.startswith('-'): neg = True; op = op[1:]
        if op.startswith('|') and op.endswith('|'): ab = True; op = op[1:-1]
        m = re.match(r'^([va])(\d+)$', op)
        if m:
            e = s.r.get(op)
            if e is None: e = ('in_' + op,); s.r[op] = e
        else:
            e = ('c', op)
        if ab: e = ('abs', e)
        if neg: e = ('neg', e)
        return e
    def regs(s, op):
        op = op.strip()
        m = re.match(r'^([va])\[(\d+):(\d+)\]$', op)
        if m: return [m.group(1) + str(i) for i in range(int(m.group(2)), int(m.group(3)) + 1)]
        m = re.match(r'^([va])(\d+)$', op)
        if m: return [op]
        return None
def split_ops(rest):
    # split on commas not inside brackets
    out=[];cur='';d=0
    for ch in rest:
        if ch=='[': d+=1
        if ch==']': d-=1
        if ch==',' and d==0: out.append(cur.strip()); cur=''
        else: cur+=ch
    if cur.strip(): out.append(cur.strip())
    return out
def run(lines):
    S = Sym()
    for raw in lines:
        l = raw.strip()
        if not l or l[0] in ';.' or l.endswith(':'): continue
        l = l.split(';')[0].strip()
        parts = l.split(None, 1)
        op = parts[0]; rest = parts[1] if len(parts) > 1 else ''
        mods = ''
        mm = re.search(r'\s(op_sel|op_sel_hi|neg_lo|neg_hi|quad_perm|row_|offen|offset|off |nt|sc\d|idxen|clamp)', ' ' + rest)
        ops = split_ops(rest)
        # strip trailing modifiers from last operand
        tail = ''
        if ops:
            m2 = re.match(r'^(\S+)\s+(.*)$', ops[-1])
            if m2: ops[-1] = m2.group(1); tail = m2.group(2)
        g = S.get
        def setr(name, e): S.r[name] = e
        if op.startswith('v_mfma'):
            for rname in S.regs(ops[0]): setr(rname, S.fresh('acc'))
        elif op in ('v_mul_f32_e32','v_mul_f32_e64'): setr(ops[0], ('mul', g(ops[1]), g(ops[2])))
        elif op in ('v_add_f32_e32','v_add_f32_e64'): setr(ops[0], ('add', g(ops[1]), g(ops[2])))
        elif op in ('v_sub_f32_e32','v_sub_f32_e64'): setr(ops[0], ('sub', g(ops[1]), g(ops[2])))
        elif op in ('v_subrev_f32_e32','v_subrev_f32_e64'): setr(ops[0], ('sub', g(ops[2]), g(ops[1])))
        elif op == 'v_fma_f32': setr(ops[0], ('fma', g(ops[1]), g(ops[2]), g(ops[3])))
        elif op in ('v_fmac_f32_e32','v_fmac_f32_e64'): setr(ops[0], ('fma', g(ops[1]), g(ops[2]), g(ops[0])))
        elif op in ('v_pk_mul_f32','v_pk_add_f32','v_pk_fma_f32'):
            nsrc = 3 if op.endswith('fma_f32') else 2
            def mod(name, dflt):
                m3 = re.search(name + r':\[([\d,]+)\]', tail)
                return [int(x) for x in m3.group(1).split(',')] if m3 else [dflt]*nsrc
            osl, osh, nlo, nhi = mod('op_sel',0), mod('op_sel_hi',1), mod('neg_lo',0), mod('neg_hi',0)
            d = S.regs(ops[0]); res=[]
            for lanei in (0,1):
                srcs=[]
                for k in range(nsrc):
                    rr = S.regs(ops[1+k])
                    sel = (osl if lanei==0 else osh)[k]
                    if rr is None: e = ('c', ops[1+k])
                    else: e = g(rr[sel] if len(rr)>1 else rr[0])
                    if (nlo if lanei==0 else nhi)[k]: e = ('neg', e)
                    srcs.append(e)
                kind = {'v_pk_mul_f32':'mul','v_pk_add_f32':'add','v_pk_fma_f32':'fma'}[op]
                res.append((kind,)+tuple(srcs))
            setr(d[0],res[0]); setr(d[1],res[1])
        elif op in ('v_mov_b32_e32','v_accvgpr_read_b32','v_accvgpr_write_b32','v_accvgpr_mov_b32'): setr(ops[0], g(ops[1]))
        elif op == 'v_mov_b32_dpp': setr(ops[0], ('dpp', g(ops[1])))
        elif op == 'v_cndmask_b32_e64' or op=='v_cndmask_b32_e32': setr(ops[0], ('sel', g(ops[1]), g(ops[2])))
        elif op in ('v_exp_f32_e32','v_rcp_f32_e32'): setr(ops[0], (op[2:5], g(ops[1])))
        elif op.startswith('buffer_load') or op.startswith('ds_read') or op.startswith('global_load'):
            for rname in (S.regs(ops[0]) or []): setr(rname, S.fresh('ld'))
        elif op.startswith('buffer_store') or op.startswith('ds_write'):
            data = ops[0] if op.startswith('buffer_store') else ops[1]
            rr = S.regs(data) or []
            S.out.append((op, [S.r.get(x, ('in_'+x,)) for x in rr]))
        elif op.startswith('v_perm_b32'):
            S.out.append(('perm', [g(ops[1]), g(ops[2])])); setr(ops[0], ('perm', g(ops[1]), g(ops[2])))
        elif op.startswith('v_') and ops and S.regs(ops[0]):
            d = S.regs(ops[0])
            e = (op[2:].split('_e')[0],) + tuple(g(o) for o in ops[1:] if S.regs(o) or re.match(r'^-?[\d.x]',o))
            for i,rname in enumerate(d): setr(rname, e if len(d)==1 else (('part%d'%i), e))
    return S
def shape(e, depth=0):
    if e[0] in ARITH: return e[0] + '(' + ','.join(shape(x, depth+1) for x in e[1:]) + ')'
    if e[0] == 'neg': return '-' + shape(e[1], depth+1)
    if e[0] == 'c': return e[1]
    if e[0] in ('rcp','exp'): return e[0]+'()' 
    if e[0].startswith('and') or e[0].startswith('lshr') or e[0].startswith('perm'): return e[0] + '[' + ','.join(shape(x,depth+1) for x in e[1:]) + ']'
    if e[0]=='sel' and depth==0: return 'sel{'+shape(e[1],1)+' | '+shape(e[2],1)+'}'
    return '_'


def table(path, pat):
    _, lines = kern(path, pat)
    S = run(lines)
    c = collections.Counter()
    for op, es in S.out:
        for e in es:
            sh = shape(e)
            if sh != '_':
                c[(op.split(' ')[0], sh)] += 1
    return c


if __name__ == '__main__':
    width = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    for k, v in sorted(table(sys.argv[1], sys.argv[2]).items()):
        print(v, k[0], k[1][:width])
