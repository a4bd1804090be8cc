'use strict';
/* Node-side checks of opts.interval on eigen_sym / eigenvals_sym, of opts.subset / opts.interval / opts.reduction on eigen_sym_gen /
 * eigenvals_sym_gen and of tridiag_eigen / tridiag_eigenvals / tridiag_count through the JS host and the N-API addon. Driven by
 * tests/test_node_eigsym_interval.py.
 *   node node_eigsym_interval_checks.js cpu                 (no GPU: the argument errors)
 *   node node_eigsym_interval_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python results)
 * Arrays travel as base64 of their bytes: the ragged results hold NaN and the bounds Infinity, which JSON has no words for. */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = s => { const b = Buffer.from(s, 'base64'); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const f64 = s => new Float64Array(bytes(s)), i32 = s => new Int32Array(bytes(s));
const nd = (shape, data) => new la.NDArray(Int32Array.from(shape), data);
const eye = N => { const d = new Float64Array(N * N); for (let i = 0; i < N; i++) d[i * N + i] = 1; return nd([N, N], d); };
const vec = (...x) => nd([x.length], Float64Array.from(x));

function argumentErrors() {
  const S = eye(4), d = vec(1, 2, 3, 4), e = vec(0, 0, 0);
  const calls = [o => la.eigen_sym(S, o), o => la.eigenvals_sym(S, o), o => la.eigen_sym_gen(S, S, o), o => la.eigenvals_sym_gen(S, S, o),
                 o => la.tridiag_eigen(d, e, o), o => la.tridiag_eigenvals(d, e, o)];
  for (const [i, f] of calls.entries()) {
    assert.throws(() => f({interval: [1, 0]}), /interval must satisfy lo <= hi/, String(i));
    assert.throws(() => f({interval: [NaN, 0]}), /interval contains NaN/, String(i));
    assert.throws(() => f({interval: [0, [1, NaN]]}), /interval must be \[lo, hi\]/, String(i));
    for (const bad of [3, [1], [0, 1, 2], 'ab', [0, 'x'], [[0, 0], 1]]) assert.throws(() => f({interval: bad}), /interval must be \[lo, hi\]/, `${i} ${JSON.stringify(bad)}`);
    assert.throws(() => f({interval: [0, 1], subset: [0, 1]}), /interval and subset exclude each other/, String(i));
    assert.throws(() => f({subset: [3, 2]}), /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= N/, String(i));
    assert.throws(() => f({subset: [2, 2]}), /the subset \[2, 2\] is empty/, String(i));
  }
  for (const f of calls.slice(0, 4)) {
    assert.throws(() => f({interval: [0, 1], algo: 'jacobi'}), /interval is not available with algo 'jacobi'/);
    assert.throws(() => f({reduction: 'sytrd'}), /reduction must be 'hessenberg' or 'tridiag'/);
  }
  for (const f of calls.slice(2, 4)) {
    assert.throws(() => f({subset: [0, 1], algo: 'jacobi'}), /subset is not available with algo 'jacobi'/);
    assert.throws(() => f({reduction: 'tridiag', algo: 'jacobi'}), /reduction is not available with algo 'jacobi'/);
  }
  assert.throws(() => la.tridiag_eigen(d, vec(0, 0)), /e must have the leading dimensions of d/);
  assert.throws(() => la.tridiag_eigen(d, null), /e must have the leading dimensions of d/);
  assert.throws(() => la.tridiag_eigenvals(vec(1), vec(1)), /null for N = 1/);
  assert.throws(() => la.tridiag_count(d, e, nd([2, 1], Float64Array.of(0, 0))), /x must have the leading dimensions of d/);
  assert.throws(() => la.tridiag_count(d, e, vec(NaN)), /x contains NaN/);
  for (const k of ['tridiag_eigen', 'tridiag_eigenvals', 'tridiag_count']) assert(typeof la[k] === 'function' && !Object.keys(la).includes(k), k);
}

// one call through host arrays and through DeviceNDArrays against the Python result
function check(name, c, call, operands) {
  const want = {lam: f64(c.lam), V: c.V ? f64(c.V) : null, range: c.range ? i32(c.range) : null};
  const keep = operands.map(o => o && Float64Array.from(o.data));
  const compare = (res, kind, Cls) => {
    const lam = c.V ? res[0] : res, V = c.V ? res[1] : null, host = x => kind === 'host' ? x : la.to_host(x);
    assert(lam instanceof Cls && (!V || V instanceof Cls), `${name} ${kind}: the kind of the result`);
    assert.deepStrictEqual(Array.from(lam.shape), c.lam_shape, `${name} ${kind}`);
    assert(sameBits(host(lam).data, want.lam), `${name} ${kind}: other values than the Python result`);
    if (V) { assert.deepStrictEqual(Array.from(V.shape), c.V_shape, `${name} ${kind}`); assert(sameBits(host(V).data, want.V), `${name} ${kind}: other vectors`); }
    if (want.range) {
      assert(res.range instanceof Cls && !Object.keys(res).includes('range'), `${name} ${kind}: range`);
      assert.deepStrictEqual(Array.from(res.range.shape), c.range_shape, `${name} ${kind}`);
      assert(sameBits(host(res.range).data, want.range), `${name} ${kind}: other ranges`);
    } else assert(res.range === undefined, `${name} ${kind}: a range without an interval`);
  };
  compare(call(operands), 'host', la.NDArray);
  operands.forEach((o, i) => o && assert(sameBits(o.data, keep[i]), `${name}: operand ${i} was written`));
  compare(call(operands.map(o => o && la.to_device(o))), 'device', la.DeviceNDArray);
}

if (mode === 'cpu') {
  argumentErrors();
  console.log('node eigsym interval cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const opts = Object.assign({}, c.opts);
    if (c.interval) opts.interval = c.interval.map(x => x === 'inf' ? Infinity : x === '-inf' ? -Infinity : typeof x === 'string' ? Array.from(f64(x)) : x);
    const ops = c.operands.map(o => o && nd(o.shape, f64(o.data)));
    if (c.fn === 'tridiag_count') {
      const want = i32(c.count);
      const got = la.tridiag_count(ops[0], ops[1], ops[2]);
      assert(got instanceof la.NDArray && got.data instanceof Int32Array && sameBits(got.data, want), name);
      const gd = la.tridiag_count(...ops.map(o => o && la.to_device(o)));
      assert(gd instanceof la.DeviceNDArray && gd.dtype === 'int32' && sameBits(la.to_host(gd).data, want), name + ' device');
    } else check(name, c, o => la[c.fn](...o, opts), ops);
    n++;
  }
  argumentErrors();
  // an interval that holds nothing throws, on both kinds; errors of the library keep their texts
  const S = eye(4), B = eye(4);
  for (const up of [x => x, x => la.to_device(x)]) {
    assert.throws(() => la.eigen_sym(up(S), {interval: [5, 6]}), /the interval holds no eigenvalue of any member/);
    assert.throws(() => la.eigenvals_sym_gen(up(S), up(B), {interval: [-Infinity, 0], reduction: 'tridiag'}), /the interval holds no eigenvalue/);
    assert.throws(() => la.tridiag_eigen(up(vec(1, 2, 3, 4)), up(vec(0, 0, 0)), {interval: [4, Infinity]}), /the interval holds no eigenvalue/);
    assert.throws(() => la.eigen_sym_gen(up(S), up(nd([4, 4], new Float64Array(16))), {subset: [0, 1]}), /B is not positive definite. \(matrix 0\)/);
    assert.throws(() => la.eigen_sym(up(nd([2, 2], Float64Array.of(1, 0, NaN, 1))), {interval: [0, 9]}), /NaN or Infinity in its lower triangle/);
    assert.throws(() => la.tridiag_eigen(up(vec(1, NaN)), up(vec(0)), {interval: [0, 9]}), /d or e contains NaN or Infinity/);
  }
  assert.throws(() => la.tridiag_eigen(la.to_device(vec(1, 2)), vec(0)), /all host arrays or all DeviceNDArrays/);
  console.log('node eigsym interval gpu checks ok', n);
} else throw new Error('mode');
