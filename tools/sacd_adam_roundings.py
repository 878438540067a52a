"""Which roundings does torch.optim.Adam use on GPU tensors?  200 000 elements, three steps, gradients over six decades: torch's result against numpy float32
emulations of the step with / without a fused multiply-add in lerp (m), in addcmul (v; 1: fma(w2 g, g, b2 v), 2: fma(w2, g g, b2 v)) and in addcdiv (p; 0: p - (s m) / d,
1: fma(-s, m / d, p), 2: p + (-s) (m / d)).  Prints the number of elements that differ per combination (lerp 1, addcmul 2, addcdiv 1 gives 0).

    python tools/sacd_adam_roundings.py > profiles/sacd_adam_roundings.txt"""
import itertools

import numpy as np
import torch

f=np.float32; d=np.float64
def fma(a,b,c): return (a.astype(d)*b.astype(d)+c.astype(d)).astype(f)
def coef(lr,b1,b2,eps,steps):
    step=steps+1; bc1=1-b1**step; bc2=1-b2**step
    return f(1-b1), f(b2), f(1-b2), f(lr/bc1), f(bc2**0.5), f(eps)
def one(p,g,m,v,c,lf,af,df):
    w1,b2,w2,ss,bs,eps=c
    m = fma(np.full_like(g,w1),(g-m),m) if lf else m+w1*(g-m)
    v = fma(w2*g,g,b2*v) if af==1 else (fma(np.full_like(g,w2),g*g,b2*v) if af==2 else b2*v+(w2*g)*g)
    denom=np.sqrt(v)/bs+eps
    if df==0: p=p-(ss*m)/denom
    elif df==1: p=fma(np.full_like(g,-ss),m/denom,p)
    else: p=p+(-ss)*(m/denom)
    return p,m,v
rng=np.random.default_rng(0)
n=200000
p0=(rng.standard_normal(n)*0.1).astype(f); gs=[(rng.standard_normal(n)*10**rng.uniform(-6,0,n)).astype(f) for _ in range(3)]
def torch_run(dev, **kw):
    tp=torch.tensor(p0.copy(),device=dev,requires_grad=True); opt=torch.optim.Adam([tp],lr=1e-3,**kw)
    for g in gs:
        tp.grad=torch.tensor(g,device=dev); opt.step()
    return tp.detach().cpu().numpy()
t=torch_run('cuda')
for lf,af,df in itertools.product((0,1),(0,1,2),(0,1,2)):
    p,m,v=p0.copy(),np.zeros(n,f),np.zeros(n,f)
    for k,g in enumerate(gs): p,m,v=one(p,g,m,v,coef(1e-3,0.9,0.999,1e-8,k),lf,af,df)
    dd=np.abs(p-t); print('lerp_fma',lf,'addcmul',af,'addcdiv',df,'mismatch',int((dd>0).sum()))
t3=torch_run('cuda',fused=True); print('gpu fused vs foreach mismatch', int((t3!=t).sum()))
