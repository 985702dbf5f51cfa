"""Two device assemblies of lariat_hip.hip, kernel by kernel: is the device code of two builds the same?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -ffp-contract=off -pthread --cuda-device-only -S -o a.s lariat_amd/csrc/lariat_hip.hip   (each build)
    python tools/cmp_device_asm.py a.s b.s

A host-only change leaves every kernel's instructions and descriptor as they were but may move kernels within the file (templates are emitted in the order the host
code first names them), so the comparison is by symbol."""
# compares two device assemblies kernel by kernel: the instructions between a symbol's label and its .Lfunc_end, and its .amdhsa_kernel descriptor block;
# local labels carry the function's ordinal in the file (.LBB45_3, .Lfunc_end45): the ordinal is dropped
import re,sys
lab=re.compile(r'(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b')
def norm(line): return lab.sub(lambda m:m.group(1)+(m.group(2) or ''),line)
def parse(path):
    body={}; desc={}; cur=None; kd=None; order=[]
    for line in open(path):
        m=re.match(r'\s*\.amdhsa_kernel\s+(\S+)',line)
        if m: kd=m.group(1); desc[kd]=[]; continue
        if kd is not None:
            if '.end_amdhsa_kernel' in line: kd=None
            else: desc[kd].append(line)
            continue
        m=re.match(r'^(_Z\w+|[A-Za-z_]\w*):\s',line)
        if m and cur is None and not m.group(1).endswith('.kd'): cur=m.group(1); body[cur]=[]; order.append(cur); continue
        if cur is not None:
            body[cur].append(norm(line))
            if line.startswith('.Lfunc_end') or re.match(r'\s*\.size\s', line): cur=None
            continue
        m=re.match(r'\s*\.amdhsa_kernel\s+(\S+)',line)
        if m: kd=m.group(1); desc[kd]=[]; continue
        if kd is not None:
            if '.end_amdhsa_kernel' in line: kd=None
            else: desc[kd].append(line)
    return body,desc,order
ba,da,oa=parse(sys.argv[1]); bb,db,ob=parse(sys.argv[2])
cuid=lambda d:{k:v for k,v in d.items() if not k.startswith('__hip_cuid_')}   # the build's identity: differs between any two compilations
ba,bb=cuid(ba),cuid(bb); oa=[k for k in oa if k in ba]; ob=[k for k in ob if k in bb]
print('functions',len(ba),len(bb),'descriptors',len(da),len(db))
print('same symbols:',set(ba)==set(bb),set(da)==set(db))
print('bodies that differ:',[k for k in ba if ba[k]!=bb.get(k)])
print('descriptors that differ:',[k for k in da if da[k]!=db.get(k)])
print('instruction lines compared:',sum(len(v) for v in ba.values()))
print('same order in the file:',oa==ob, 'symbols out of place:',sum(1 for x,y in zip(oa,ob) if x!=y))
