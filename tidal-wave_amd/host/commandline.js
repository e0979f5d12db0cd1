#!/usr/bin/env node
// commandline.js — the CLI contract of the reference (/root/reference/commandline.js:2-19,41-59): options
// -threshold -span -pyrScale -pyrLevels -winSize -pyrIterations -polyN -polySigma -flags, two positional
// paths, pretty JSON per result on stdout.  Not in the reference: -ignore x,y,w,h (repeatable), a region of every pair
// that may differ; -regions N (1 .. 8), the vectors of every pair grouped into regions (`regions` behind `vector`, `region`
// in every vector), N being the gap in grid steps that still joins two vectors; -residual N (1 .. 254), the cells of every pair
// with a pixel that differs by more than N gray levels and how many of those the flow does not explain (`change` behind the
// other keys), and -residualMin N, which makes a pair with at least N unexplained pixels SUSPICIOUS even without a vector; -shift N (1 .. 1024),
// every pair's flow started from its global shift of at most N pixels, found on the device (`shift` behind the other keys); -shiftBands N (32 .. 1024, a multiple of 16; with -shift), one vertical shift
// per band of N rows instead (`bands` behind `shift`);
// -overlay DIR, a diff image of every SUSPICIOUS pair, rendered on the device and written to DIR (created if missing) as a PNG
// whose path is the result's last key `overlay`, and -overlayTol N (0 .. 255, default 16), the gray-level difference above
// which a pixel is painted as changed.  The reference's own script cannot run (it requires
// './opticalflow.js', which does not exist, commandline.js:62); this one drives index.js.  No stdout dup2
// trick is needed: the native layer here does not print.
// expect_path / target_path may be two directories (every file of target is paired with the same relative
// path under expect) or two image files.
'use strict';
var FS = require('fs');
var Path = require('path');

var usage =
  '[USAGE]\n' +
  '  node commandline.js [options] expect_path target_path\n' +
  '\n' +
  'ex)\n' +
  '  $ node commandline.js -threshold 1.0 -span 10 test/images test/images2\n';

var supportedOptions = ['threshold', 'span', 'pyrScale', 'pyrLevels', 'winSize', 'pyrIterations', 'polyN',
  'polySigma', 'flags', 'numThreads', 'regions', 'residual', 'residualMin', 'shift', 'shiftBands', 'overlayTol'];

function getArgs(argv) {
  var positional = [], options = {};
  for (var i = 0; i < argv.length; i++) {
    var m = /^--?([A-Za-z]+)(?:=(.*))?$/.exec(argv[i]);
    if (m && m[1] === 'ignore') {
      var r = parseRegion(m[2] !== undefined ? m[2] : argv[++i]);
      if (!r) { process.stderr.write('-ignore takes x,y,w,h (four integers)\n' + usage); process.exit(-1); }
      (options.ignore = options.ignore || []).push(r);
    } else if (m && m[1] === 'overlay') {
      options.overlay = Path.resolve(String(m[2] !== undefined ? m[2] : argv[++i]));   // a directory, not a number
    } else if (m && supportedOptions.indexOf(m[1]) !== -1) {
      var v = m[2] !== undefined ? m[2] : argv[++i];
      options[m[1]] = Number(v);          // numbers, like minimist does for numeric-looking values
    } else {
      positional.push(argv[i]);
    }
  }
  if (positional.length < 2) { process.stderr.write(usage); process.exit(-1); }
  return { expect_path: positional[0], target_path: positional[1], options: options };
}

// "x,y,w,h" -> {x, y, width, height}; null unless it is four integers (x and y may be negative)
function parseRegion(s) {
  var m = /^(-?\d+),(-?\d+),(-?\d+),(-?\d+)$/.exec(String(s));
  return m ? { x: Number(m[1]), y: Number(m[2]), width: Number(m[3]), height: Number(m[4]) } : null;
}

function print(o) { process.stdout.write(JSON.stringify(o, null, '  ') + '\n'); }

function main(args) {
  var TW = require('./index');
  if (args.options.overlay) FS.mkdirSync(args.options.overlay, { recursive: true });
  var isDir = false;
  try { isDir = FS.statSync(args.target_path).isDirectory(); } catch (e) { /* reported as an ERROR response */ }
  var t;
  if (isDir) {
    var opts = {};
    Object.keys(args.options).forEach(function(k) { opts[k] = args.options[k]; });
    opts.expectDir = args.expect_path;
    t = TW.create(args.target_path, opts);
  } else {
    t = new TW.TidalWave(args.options);
    t.on('data', function() { t.dispose(); });
    t.on('error', function() { t.dispose(); });
    if (args.options.ignore) t.calcIgnoring(Path.resolve(args.expect_path), Path.resolve(args.target_path), args.options.ignore);
    else t.calc(Path.resolve(args.expect_path), Path.resolve(args.target_path));
  }
  t.on('data', print);
  t.on('error', print);
  t.once('finish', print);
}

module.exports.getArgs = getArgs;
if (require.main === module) main(getArgs(process.argv.slice(2)));
